"""What the PSNR / SSIM of run.run_movement cost per frame, on the host (MetricsWriter.append) and on the device
(cfg.amd.metrics = 'device': hnrf_image_metrics in the frame's launches), and the kernel pass on its own.
    python profiles/tools/time_metrics.py [n_frames] > profiles/device_metrics.txt
The driver starts every step as a child process of its own under a time limit and stops at the first that fails:
    op      ops.image_metrics by device events, 512^2 and 1024^2, with and without a mask
    exact   run_movement on a 512^2 synthetic subject four ways, alternating, each twice: no metrics | ['psnr'] host |
            ['psnr', 'ssim'] host | ['psnr', 'ssim'] device
    baked   the same loop with cfg.amd.canonical = cfg.amd.nonrigid = 'baked', where host metrics weigh most
Per way: ms per frame of both repeats and their spread, the medians of render_frames.last_prefetch['on_image_ms'] and
['gpu_gap_ms'] (cfg.amd.loop_timing)."""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STEPS = (('op', 240), ('exact', 420), ('baked', 420))


def step_op():
    import numpy as np, torch
    from humannerf_amd import ops
    dev = torch.device('cuda:0')
    for size in (512, 1024):
        g = torch.Generator(device='cpu').manual_seed(size)
        a = torch.randint(0, 256, (size, size, 3), generator=g, dtype=torch.uint8).to(dev)
        b = (a.int() + torch.randint(-9, 10, (size, size, 3), generator=g).to(dev)).clamp(0, 255).to(torch.uint8)
        m = torch.zeros(size, size, dtype=torch.uint8, device=dev)
        m[size // 8 + 1:size - size // 8, size // 4 + 3:size - size // 4] = 1
        for mask in (None, m):
            for _ in range(20):
                out = ops.image_metrics(a, b, mask)
            torch.cuda.synchronize()
            reps, calls, ms = 5, 200, []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    out = ops.image_metrics(a, b, mask)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / calls)
            print('ops.image_metrics %4d^2 %-9s: %.1f us per call (4 launches; device events over %d x %d calls, median; '
                  'min %.1f max %.1f); psnr %.4f ssim %.6f' % (size, 'masked' if mask is not None else 'no mask',
                  1e3 * float(np.median(ms)), reps, calls, 1e3 * min(ms), 1e3 * max(ms), *out[0].tolist()), flush=True)


def step_loop(baked, n):
    import numpy as np, torch
    from humannerf_amd import dataset, render, run, scene
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state
    d = tempfile.mkdtemp()
    scene.write_synthetic_subject(d, n_frames=n, size=512, binary_mask=True)
    cfg.resize_img_scale = 1.0
    cfg.N_samples, cfg.perturb, cfg.amd.diagnostics, cfg.amd.loop_timing = 128, 0., False, True
    if baked:
        cfg.amd.canonical, cfg.amd.nonrigid = 'baked', 'baked'
    dev = torch.device('cuda:0')
    subj = dataset.Subject(d)
    net = Network(); net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state(default_shapes(), 0).items()})
    net = net.to(dev).eval()
    out = tempfile.mkdtemp()
    # (no metrics: the device route with an empty list -- nothing is enqueued and MetricsWriter.append is not called)
    ways = (('no metrics', 'device', []), ("['psnr'] host", 'host', ['psnr']), ("['psnr','ssim'] host", 'host', ['psnr', 'ssim']),
            ("['psnr','ssim'] device", 'device', ['psnr', 'ssim']))
    for _, route, metrics in ways[2:]:                                                   # warm-up: two frames per route
        cfg.amd.metrics = route
        run.run_movement(net, subj, render_folder_name='warm_' + route, logdir=out, device=dev, test_num=2, metrics=metrics)
    res = {w[0]: [] for w in ways}
    for rep in range(2):
        for name, route, metrics in ways:
            cfg.amd.metrics = route
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = run.run_movement(net, subj, render_folder_name='t%d_%d' % (rep, len(metrics) * 2 + (route == 'device')),
                                 logdir=out, device=dev, metrics=metrics)
            torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3 / n
            lp = render.render_frames.last_prefetch
            res[name].append((ms, float(np.median(lp['on_image_ms'])), float(np.median(lp['gpu_gap_ms'])),
                              float(np.median(lp['gpu_ms'])), float(np.median(lp['image_wait_ms'])), r['metrics']))
    title = 'baked renderer (canonical = nonrigid = baked)' if baked else 'exact renderer'
    print('%s, %d frames of 512^2, run_movement with PNG writer; per way two alternating repeats' % (title, n))
    base = res['no metrics']
    spread0 = abs(base[0][0] - base[1][0])
    for name, _, _ in ways:
        a, b = res[name]
        print('  %-24s %7.2f | %7.2f ms per frame (spread %.2f); medians of the second repeat: on_image %.2f ms, gpu busy %.2f ms, '
              'gpu gap %.2f ms, wait for image %.2f ms; averages %s'
              % (name, a[0], b[0], abs(a[0] - b[0]), b[1], b[3], b[2], b[4], {k: round(v, 4) for k, v in (b[5] or {}).items()}))
    mean = lambda k: 0.5 * (res[k][0][0] + res[k][1][0])
    dv, no, hs = mean("['psnr','ssim'] device"), mean('no metrics'), mean("['psnr','ssim'] host")
    print('  device route - no metrics = %+.2f ms per frame (spread of the two no-metrics repeats: %.2f ms): %s; '
          "host ['psnr','ssim'] / device = %.2fx" % (dv - no, spread0, 'within' if abs(dv - no) <= spread0 else 'OUTSIDE', hs / dv),
          flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--step':
        n = int(sys.argv[3]) if len(sys.argv) > 3 else 24
        {'op': step_op, 'exact': lambda: step_loop(False, n), 'baked': lambda: step_loop(True, n)}[sys.argv[2]]()
        sys.exit(0)
    n = sys.argv[1] if len(sys.argv) > 1 else '24'
    for step, limit in STEPS:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, n], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print('step %s ended with status %d: stopping' % (step, rc), flush=True)
            sys.exit(rc if rc > 0 else 1)
