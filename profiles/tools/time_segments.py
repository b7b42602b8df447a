"""What splitting the surface records by body part costs, on the records of time_cloud.py (seeded network, synthetic
subject).
    python profiles/tools/time_segments.py [n_frames=16] [size=512] > profiles/segments.txt
One process, device events around the launches (medians of 5 repeats; the compaction's read-back of the counts lies
inside the events), every step printed as it ends:
    records   run.run_surface_points over the movement frames, wall per frame: what a frame's records cost to produce
    segment   hnrf_segment_members and the compaction (hnrf_segment_count + _scatter), one frame and the batch, all 15
              parts; cloud.segment_records (pack, kernels, one gather per part, copy to the host) by the wall clock
    fused     cloud.segment_distance_matrices (one pack, P F clouds, one pairs call) against the route it replaces,
              fifteen cloud.distance_matrix calls on the segmented records -- alternating, wall clock around a
              synchronise, the segments given as segment_records returns them (host tensors) and already on the device
    eager     the comparator: the computation of tools/segment.py:33-48 for one frame and all 15 parts, run eagerly by
              PyTorch on the same GPU in the tool's own formulation (the (N, M, 2) tensor of pixel differences between
              all records and a part's seeds, its L1 sum, the minimum over the seeds, the boolean gather), on a frame
              cut to TARGET records so that the tensor fits; our kernels on the same records beside it, and the two
              selections compared
The seeded network is no trained body (time_cloud.py): the records are taken with threshold 0 where fewer than 10 000
rays per frame pass 0.3 (so nearly every pixel of the image carries a record, where a trained body covers its
silhouette), its arg-max bones follow the subject's weight volume, not a trained field (the output prints how many
occur and how many parts a record belongs to), and the distance's weight filter is the value that keeps TARGET points
of the first frame."""
import os, sys, tempfile, time
TARGET = 49152
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_cloud import events_ms


def wall_ms(fn, reps=5):
    import numpy as np, torch
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) * 1e3)
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
        torch.cuda.synchronize(); records_ms = (time.perf_counter() - t0) * 1e3 / n
        counts = [int(r.shape[0]) for r in res['records'].values()]
        print('records: %d frames of %d^2, weight threshold %g: %.1f ms per frame (wall, whole loop); records per frame min %d '
              'median %d max %d' % (n, size, thr, records_ms, min(counts), int(np.median(counts)), max(counts)), flush=True)
        if np.median(counts) >= 10000 or thr == 0.0:
            break
        print('  (the seeded network puts fewer than 10 000 rays per frame over 0.3: records taken with threshold 0)')
        thr = 0.0
    recs = res['records']
    names = sorted(recs)
    vwt = thr
    if thr == 0.0 and recs[names[0]].shape[0] > TARGET:
        vwt = float(torch.sort(recs[names[0]][:, 6], descending=True)[0][TARGET])
        print('  (distance: weight filter %.6g, which keeps %d records of the first frame)' % (vwt, TARGET))
    F, P = len(names), len(cloud.BODY_PARTS)
    masks = torch.from_numpy(cloud.bone_masks().view(np.int32)).to(dev)
    frames = [recs[k].to(dev) for k in names]
    lbs = torch.cat([f[:, 9] for f in frames]).long()
    print('bones: %d distinct arg-max bones over the batch; share of the most frequent %.2f'
          % (int(torch.unique(lbs).numel()), float(torch.bincount(lbs).max()) / max(1, lbs.numel())), flush=True)

    # ---- the kernels: one frame, the batch
    for what, fs in (('one frame', frames[:1]), ('batch of %d frames' % F, frames)):
        rec, offsets = cloud._segment_pack(fs, dev)
        m = events_ms(lambda: ops.segment_members(rec, offsets, masks, size, size, 10))
        member, status = ops.segment_members(rec, offsets, masks, size, size, 10)
        c = events_ms(lambda: ops.segment_compact(member, offsets, P, status=status))
        seg, src = ops.segment_compact(member, offsets, P, status=status)
        both = events_ms(lambda: ops.segment_compact(*ops.segment_members(rec, offsets, masks, size, size, 10)[:1], offsets, P))
        print('segment, %s (%d records, %d^2, radius 10, %d parts): members %.3f ms (min %.3f max %.3f), compaction '
              '%.3f ms (min %.3f max %.3f), both %.3f ms = %.3f ms per frame; %d rows kept = %.2f parts per record'
              % (what, rec.shape[0], size, P, *m, *c, both[0], both[0] / len(fs), src.numel(), src.numel() / max(1, rec.shape[0])),
              flush=True)
        segment_ms = both[0] / len(fs)
    w = wall_ms(lambda: cloud.segment_records(recs, image_size=(size, size)), reps=3)
    print('cloud.segment_records, %d frames from host tensors to host tensors (pack, kernels, %d gathers, copies): %.1f ms '
          '(min %.1f max %.1f) = %.1f ms per frame (wall)' % (F, P, *w, w[0] / F), flush=True)
    print('CHECK segmenting a frame (%.3f ms, kernels; %.1f ms with the copies both ways) against producing its records '
          '(%.1f ms): %s' % (segment_ms, w[0] / F, records_ms, 'less' if w[0] / F < records_ms else 'NOT LESS'), flush=True)

    # ---- fused matrices against fifteen distance_matrix calls
    axis = cloud.default_axis([f[f[:, 6] > vwt][:, :3].cpu().numpy() for f in frames])
    seg_host = cloud.segment_records(recs, image_size=(size, size))
    seg_dev = {p: {k: (None if v is None else v.to(dev)) for k, v in s.items()} for p, s in seg_host.items()}
    dev_recs = dict(zip(names, frames))
    for tau in (0.002, 0.02):
        kw = dict(valid_weight_threshold=vwt, dist_thresh=tau, axis=axis)
        fused = lambda r: cloud.segment_distance_matrices(r, image_size=(size, size), **kw)
        fifteen = lambda s: {p: cloud.distance_matrix(s[p], **kw) for p in cloud.BODY_PARTS}
        a, b = fused(recs), fifteen(seg_host)                                            # warm-up, and the comparison
        same = all(np.array_equal(a[p], b[p]) for p in cloud.BODY_PARTS)
        t = {k: [] for k in ('fused, host records', 'fused, device records', 'fifteen calls, host segments',
                             'fifteen calls, device segments')}
        for _ in range(5):                                                               # alternating
            t['fused, host records'].append(wall_ms(lambda: fused(recs), reps=1)[0])
            t['fifteen calls, host segments'].append(wall_ms(lambda: fifteen(seg_host), reps=1)[0])
            t['fused, device records'].append(wall_ms(lambda: fused(dev_recs), reps=1)[0])
            t['fifteen calls, device segments'].append(wall_ms(lambda: fifteen(seg_dev), reps=1)[0])
        print('matrices, %d parts x %d pairs, tau %g, weight filter %.6g, axis %d; equal as float32 arrays: %s; mean D %.2f'
              % (P, F * (F - 1) // 2, tau, vwt, axis, same, float(np.mean([a[p].mean() for p in a]))), flush=True)
        for k, v in t.items():
            print('  %-32s %9.1f ms (min %.1f max %.1f; wall, medians of 5)' % (k, float(np.median(v)), min(v), max(v)), flush=True)
        med = {k: float(np.median(v)) for k, v in t.items()}
        print('CHECK tau %g: fused %.1f ms against fifteen calls %.1f ms (records and segments on the device: the fifteen '
              'calls do not count the segmentation that made their input): %s' % (
                  tau, med['fused, device records'], med['fifteen calls, device segments'],
                  'not slower' if med['fused, device records'] <= med['fifteen calls, device segments'] else 'SLOWER'), flush=True)

    # ---- the reference's expressions, eagerly, on one frame cut to TARGET records
    f0 = frames[0]
    if f0.shape[0] > TARGET:
        f0 = f0[torch.sort(torch.sort(f0[:, 6], descending=True)[1][:TARGET])[0]].contiguous()
    pos, bone = f0[:, 7:9], f0[:, 9]

    def eager():
        kept = []
        for ls in cloud.BODY_PARTS.values():
            seeds = torch.isin(bone, torch.tensor(ls, dtype=bone.dtype, device=dev))
            if not bool(seeds.any()):
                kept.append(None)
                continue
            l1 = (pos[:, None, :] - pos[seeds][None, :, :]).abs().sum(dim=-1)             # through the (N, M, 2) tensor
            kept.append(f0[l1.min(dim=1)[0] < 10])
        return kept
    seeds = [int(torch.isin(bone, torch.tensor(ls, dtype=bone.dtype, device=dev)).sum()) for ls in cloud.BODY_PARTS.values()]
    if f0.shape[0] * max(seeds) * 8 * 3 < 60e9:
        e = events_ms(eager, reps=5)
        rec, offsets = cloud._segment_pack([f0], dev)
        ours = events_ms(lambda: ops.segment_compact(*ops.segment_members(rec, offsets, masks, size, size, 10)[:1], offsets, P))
        seg, src = ops.segment_compact(*ops.segment_members(rec, offsets, masks, size, size, 10)[:1], offsets, P)
        ref = eager()
        same = all((r is None and seg[p + 1] == seg[p]) or (r is not None and torch.equal(r, rec[src[seg[p]:seg[p + 1]].long()]))
                   for p, r in enumerate(ref))
        print('eager: the reference\'s formulation, one frame of %d records (seeds per part %d .. %d), 15 parts: %.2f ms '
              '(min %.2f max %.2f); members + compaction on the same records: %.3f ms (min %.3f max %.3f) = %.0fx; '
              'same rows: %s' % (f0.shape[0], min(seeds), max(seeds), *e, *ours, e[0] / ours[0], same), flush=True)
    else:
        print('eager: skipped (the N x M x 2 intermediates exceed 60 GB)', flush=True)


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 16, int(sys.argv[2]) if len(sys.argv) > 2 else 512)
