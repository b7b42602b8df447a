"""What the Motion-JPEG output of the render loops costs (cfg.amd.video, humannerf_amd/video.py, csrc/hnrf_video.hip).
    python profiles/tools/time_video.py [n_frames] > profiles/video_encode.txt
The driver starts every step as a child process of its own under a time limit and stops at the first that fails:
    op      JpegEncoder.encode (three launches) alone by device events, 5 x 200 = 1 000 calls, 512 x 512 and 512 x 1536,
            on a rendered-looking image (smooth body on a flat background) and on uniform noise, quality 90
    loop    run_movement on a 512^2 synthetic subject with cfg.amd.canonical = cfg.amd.nonrigid = 'baked', four ways,
            alternating, each twice: no writer (ImageWriter replaced by one that drops the images) | PNG writer (the loop
            without this option) | video = 'mjpeg' | video = 'mjpeg_only'; panels [render | truth], no metrics
Per way: ms per frame of both repeats and their spread, the bytes copied to the host per frame (from the shapes; the
video's from render_frames.last_video), the stream's mean size and the number of copy-cap fall-backs."""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STEPS = (('op', 240), ('loop', 480))


def _picture(H, W, noise):
    import numpy as np
    rs = np.random.RandomState(H + W)
    if noise:
        return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.full((H, W, 3), (30., 120., 250.))
    for p in range(W // 512):                                            # one soft, textured blob per 512-wide panel
        cx, cy = 256 + 512 * p, H / 2
        body = np.exp(-(((x - cx) / 90) ** 2 + ((y - cy) / 190) ** 2) ** 3)[..., None]
        tex = np.stack([150 + 60 * np.sin(x / 7 + p), 110 + 50 * np.cos(y / 11), 90 + 40 * np.sin((x + y) / 5)], -1)
        img = img * (1 - body) + (tex + rs.normal(0, 4, (H, W, 3))) * body
    return img.clip(0, 255).astype(np.uint8)


def step_op():
    import numpy as np, torch
    from humannerf_amd import video
    dev = torch.device('cuda:0')
    enc = video.JpegEncoder(dev, 90)
    for H, W in ((512, 512), (512, 1536)):
        for noise in (False, True):
            host = _picture(H, W, noise)
            img = torch.from_numpy(host).to(dev)
            for _ in range(20):
                buf, n = enc.encode(img)
            torch.cuda.synchronize()
            assert buf[:int(n.item())].cpu().numpy().tobytes() == video.jpeg_encode_numpy(host, 90)
            reps, calls, ms = 5, 200, []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    buf, n = enc.encode(img)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / calls)
            print('JpegEncoder.encode %4d x %4d q90 %-8s: %.1f us per call (3 launches + the two result allocations; device '
                  'events over %d x %d calls, median; min %.1f max %.1f); stream %d bytes = %.2f bits per pixel; equal to the twin'
                  % (H, W, 'noise' if noise else 'rendered', 1e3 * float(np.median(ms)), reps, calls, 1e3 * min(ms), 1e3 * max(ms),
                     int(n.item()), 8.0 * int(n.item()) / (H * W)), flush=True)


class _NullWriter:
    """ImageWriter's interface with nothing behind it: the loop without a writer."""

    def __init__(self, output_dir, exp_name, **kw):
        self.image_dir = os.path.join(output_dir, exp_name)

    def append(self, image, img_name=None):
        return 0, img_name

    def finalize(self, video_name=None):
        return None


def step_loop(n):
    import numpy as np, torch
    from humannerf_amd import dataset, render, run, scene
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state
    d = tempfile.mkdtemp()
    scene.write_synthetic_subject(d, n_frames=n, size=512, binary_mask=True)
    cfg.resize_img_scale = 1.0
    cfg.N_samples, cfg.perturb, cfg.amd.diagnostics, cfg.amd.loop_timing = 128, 0., False, True
    cfg.amd.canonical, cfg.amd.nonrigid, cfg.amd.metrics = 'baked', 'baked', 'device'
    dev = torch.device('cuda:0')
    subj = dataset.Subject(d)
    net = Network(); net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state(default_shapes(), 0).items()})
    net = net.to(dev).eval()
    out = tempfile.mkdtemp()
    real_writer = render.ImageWriter
    ways = (('no writer', 'none', _NullWriter), ('PNG writer', 'none', real_writer), ("video = 'mjpeg'", 'mjpeg', real_writer),
            ("video = 'mjpeg_only'", 'mjpeg_only', real_writer))

    def one(tag, mode, writer, frames):
        cfg.amd.video = mode
        render.ImageWriter = writer
        try:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = run.run_movement(net, subj, render_folder_name=tag, logdir=out, device=dev, test_num=frames, metrics=[])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / frames, r
        finally:
            render.ImageWriter = real_writer

    for k, (_, mode, writer) in enumerate(ways):                                          # warm-up: two frames per way
        one('warm_%d' % k, mode, writer, 2)
    res = {w[0]: [] for w in ways}
    H = W = 512
    for rep in range(2):
        for k, (name, mode, writer) in enumerate(ways):
            ms, r = one('t%d_%d' % (rep, k), mode, writer, n)
            lp, lv = render.render_frames.last_prefetch, dict(render.render_frames.last_video)
            image_bytes = 0 if mode == 'mjpeg_only' else 3 * H * W * 3                      # rgb, alpha, truth: 8 bit, 3 channels
            video_bytes = (lv['cap'] + 8) if mode != 'none' else 0
            size = os.path.getsize(r['video']) if r.get('video') else 0
            res[name].append((ms, float(np.median(lp['gpu_ms'])), float(np.median(lp['gpu_gap_ms'])), image_bytes + video_bytes,
                              lv, size))
    print("baked renderer (canonical = nonrigid = 'baked'), %d frames of 512^2, run_movement, panels [render | truth] = 512 x 1024, "
          'quality 90; per way two alternating repeats' % n)
    for name, _, _ in ways:
        a, b = res[name]
        lv = b[4]
        print('  %-22s %7.2f | %7.2f ms per frame (spread %.2f); second repeat: gpu busy %.2f ms, gpu gap %.2f ms (medians); '
              '%d bytes to the host per frame%s' % (name, a[0], b[0], abs(a[0] - b[0]), b[1], b[2], b[3],
              '' if not lv['frames'] else '; stream %.0f bytes per frame on average, copy cap %d, fall-backs %d of %d, file %d bytes'
              % (lv['bytes'] / lv['frames'], lv['cap'], lv['fallbacks'], lv['frames'], b[5])))
    mean = lambda k: 0.5 * (res[k][0][0] + res[k][1][0])
    lo, hi = sorted(x[0] for x in res['no writer'])
    only = [x[0] for x in res["video = 'mjpeg_only'"]]
    inside = all(lo <= x <= hi for x in only)
    print("  expectation 'mjpeg_only sits inside the spread of the two no-writer repeats' [%.2f, %.2f]: %s (%.2f | %.2f); "
          "mjpeg_only - no writer = %+.2f ms, mjpeg - PNG writer = %+.2f ms, PNG writer - no writer = %+.2f ms (means of two)"
          % (lo, hi, 'CONFIRMED' if inside else 'REFUTED', only[0], only[1], mean("video = 'mjpeg_only'") - mean('no writer'),
             mean("video = 'mjpeg'") - mean('PNG writer'), mean('PNG writer') - mean('no writer')), flush=True)
    print('  not measured: playback in a real player (none on the machine; PIL decodes every chunk in the tests); parity '
          "with the reference's MP4 (another codec)", flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--step':
        n = int(sys.argv[3]) if len(sys.argv) > 3 else 24
        {'op': step_op, 'loop': lambda: step_loop(n)}[sys.argv[2]]()
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
