"""What the surface-point records and the frame x frame distance cost on the seeded network and a synthetic subject.
    python profiles/tools/time_cloud.py [n_frames=16] [size=512] > profiles/cloud_distance.txt
One process, device events around the launches (medians of 5 repeats), every step printed as it ends:
    records   run.run_surface_points over the movement frames (forward with the eleven outputs + hnrf_surface_points +
              the copy of the records to the host), and hnrf_surface_points alone on one frame's outputs
    nn        hnrf_cloud_nn, frame 0 against frame 1, one direction
    window    hnrf_cloud_distance_pairs, all F (F - 1) / 2 pairs in one call, tau = 0.002 and 0.02 (sorting and packing
              the frames once is timed separately)
    brute     the same matrix by two hnrf_cloud_nn launches per pair (kernel time only)
    eager     the comparator: the reference's expressions of find_nearest_pair_gpu / compute_distance_gpu run eagerly by
              PyTorch on the same GPU -- the full N0 x N1 fp32 distance matrix, two argmins, the gather and the
              non-zero test, colour errors and threshold vectorised (the reference's Python loop over the pairs is
              left out) -- on the first 8 pairs, scaled to the matrix
The seeded network is no trained body: where fewer than 10 000 rays per frame pass weight max > 0.3 the records are
taken with threshold 0 and the distance's weight filter is set to the value that keeps TARGET points of the first
frame (column 6 is the weight max), so that the clouds have the size of a trained body's; the output says so."""
import os, sys, tempfile, time
TARGET = 49152
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def events_ms(fn, reps=5):
    import numpy as np, torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def main(n, size):
    import numpy as np, torch
    from humannerf_amd import cloud, dataset, ops, run, scene
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state
    d, out = tempfile.mkdtemp(), tempfile.mkdtemp()
    scene.write_synthetic_subject(d, n_frames=n, size=size, binary_mask=True)
    cfg.resize_img_scale = 1.0
    cfg.N_samples, cfg.perturb = 128, 0.
    dev = torch.device('cuda:0')
    subj = dataset.Subject(d)
    net = Network(); net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state(default_shapes(), 0).items()})
    net = net.to(dev).eval()
    run.run_surface_points(net, subj, logdir=out, device=dev, test_num=2)                # warm-up
    thr = 0.3
    for attempt in range(2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = run.run_surface_points(net, subj, weight_threshold=thr, logdir=out, device=dev)
        torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3 / n
        counts = [int(r.shape[0]) for r in res['records'].values()]
        print('records: %d frames of %d^2, weight threshold %g: %.1f ms per frame (wall, whole loop); points per frame min %d '
              'median %d max %d' % (n, size, thr, ms, min(counts), int(np.median(counts)), max(counts)), flush=True)
        if np.median(counts) >= 10000 or thr == 0.0:
            break
        print('  (the seeded network puts fewer than 10 000 rays per frame over 0.3: records taken with threshold 0)')
        thr = 0.0
    recs = res['records']
    names = sorted(recs)
    vwt = thr
    if thr == 0.0 and recs[names[0]].shape[0] > TARGET:
        vwt = float(torch.sort(recs[names[0]][:, 6], descending=True)[0][TARGET])
        print('  (distance: weight filter %.6g, which keeps %d points of the first frame)' % (vwt, TARGET))
    R, S, B = 65536, 128, 24
    g = torch.Generator().manual_seed(0)
    w, xyz, bmw = torch.rand(R, S, generator=g).to(dev), torch.randn(R, S, 3, generator=g).to(dev), torch.rand(R, S, B, generator=g).to(dev)
    m = events_ms(lambda: ops.surface_points(w, xyz, bmw))
    print('hnrf_surface_points alone, %d rays x %d samples x %d bones: %.3f ms (min %.3f max %.3f); %.0f MB read -> %.2f TB/s'
          % (R, S, B, *m, R * S * (1 + 3 + B) * 4 / 1e6, R * S * (1 + 3 + B) * 4 / m[0] / 1e9), flush=True)

    frames = [recs[k].to(dev) for k in names]
    frames = [f[f[:, 6] > vwt] for f in frames]
    print('clouds: points per frame min %d median %d max %d' % (min(f.shape[0] for f in frames), int(np.median([f.shape[0] for f in frames])), max(f.shape[0] for f in frames)), flush=True)
    xyzs, rgbs = [f[:, :3].contiguous() for f in frames], [f[:, 3:6].contiguous() for f in frames]
    axis = cloud.default_axis([x.cpu().numpy() for x in xyzs])
    F = len(frames)
    pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]
    m = events_ms(lambda: ops.cloud_nn(xyzs[0], xyzs[1]))
    print('hnrf_cloud_nn: %d x %d points: %.3f ms (min %.3f max %.3f) = %.1f G pair distances / s'
          % (xyzs[0].shape[0], xyzs[1].shape[0], *m, xyzs[0].shape[0] * xyzs[1].shape[0] / m[0] / 1e6), flush=True)
    m = events_ms(lambda: cloud._pack(xyzs, axis, dev, colours=rgbs))
    pk = cloud._pack(xyzs, axis, dev, colours=rgbs)
    print('sort and pack %d frames once (torch.sort along axis %d): %.3f ms' % (F, axis, m[0]), flush=True)
    pt = torch.tensor(pairs, dtype=torch.int32, device=dev)
    D = {}
    for tau in (0.002, 0.02):
        m = events_ms(lambda: ops.cloud_distance_pairs(pk['xyz'], pk['rgb'], pk['orig'], pk['offsets'], pt, tau, axis, pk['max_n']))
        D[tau] = ops.cloud_distance_pairs(pk['xyz'], pk['rgb'], pk['orig'], pk['offsets'], pt, tau, axis, pk['max_n'])[0].cpu().numpy()
        print('window: hnrf_cloud_distance_pairs, %d pairs, tau %g: %.3f ms (min %.3f max %.3f) = %.4f ms per pair; '
              'mean D %.4f, pairs with D > 0: %d' % (len(pairs), tau, *m, m[0] / len(pairs), D[tau].mean(), (D[tau] > 0).sum()),
              flush=True)

    def brute_all():
        for i, j in pairs:
            ops.cloud_nn(xyzs[i], xyzs[j]); ops.cloud_nn(xyzs[j], xyzs[i])
    m = events_ms(brute_all, reps=3)
    print('brute: 2 x hnrf_cloud_nn per pair, %d pairs: %.3f ms (min %.3f max %.3f) = %.4f ms per pair (threshold and '
          'colour errors not included)' % (len(pairs), *m, m[0] / len(pairs)), flush=True)
    brute_ms = m[0]

    def eager(i, j, tau):
        dist = torch.linalg.norm(xyzs[i][:, None, :] - xyzs[j][None, :, :], axis=-1)
        min0, min1 = torch.argmin(dist, axis=1), torch.argmin(dist, axis=0)
        pair_0 = (min1[min0] == torch.arange(xyzs[i].shape[0], device=dev)).nonzero().reshape(-1)
        pair_1 = min0[pair_0]
        err = torch.linalg.norm(rgbs[i][pair_0] - rgbs[j][pair_1], axis=-1)
        return torch.sum(err * (dist[pair_0, pair_1] < tau))
    some = [p for p in pairs if xyzs[p[0]].shape[0] * xyzs[p[1]].shape[0] * 16 < 60e9][:8]
    if some and all(xyzs[i].shape[0] and xyzs[j].shape[0] for i, j in some):
        for tau in (0.002, 0.02):
            m = events_ms(lambda: [eager(i, j, tau) for i, j in some], reps=3)
            vals = np.array([float(eager(i, j, tau)) for i, j in some])
            ours = np.array([D[tau][pairs.index(p)] for p in some])
            print('eager: PyTorch on the same GPU, %d pairs, tau %g: %.3f ms per pair (min %.3f max %.3f), x %d pairs = %.1f ms; '
                  'max |eager - window| / max(1, D) = %.2g' % (len(some), tau, m[0] / len(some), m[1] / len(some), m[2] / len(some),
                  len(pairs), m[0] / len(some) * len(pairs), float(np.max(np.abs(vals - ours) / np.maximum(1, ours)))), flush=True)
    else:
        print('eager: skipped (empty frames, or the N0 x N1 x 3 intermediate exceeds 60 GB)', flush=True)
    print('brute kernel / window at tau 0.002: see the two lines above (%.3f ms for the brute matrix)' % brute_ms, flush=True)


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 16, int(sys.argv[2]) if len(sys.argv) > 2 else 512)
