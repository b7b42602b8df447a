"""What the density-gradient normals cost and how they compare with the screen-space ones and with the mesh
(cfg.amd.maps_normals, include/hnrf_normals.h, csrc/hnrf_normals.hip, Network.ray_normals / vertex_normals).
    python profiles/tools/time_normals.py [n_frames] > profiles/normals.txt
The driver starts every step as a child process of its own under a time limit and stops at the first that fails:
    frame   the bench frame (512 x 512 rays of 128 samples, scene.synthetic_frame, the seeded network with the sigma bias
            raised by 5) rendered with diagnostics: the share of samples kept at weight_min = 1e-4; by device events,
            5 repeats each: the compaction, the gradient pass (ops.density_gradient with the non-rigid chain),
            hnrf_ray_normals, hnrf_normal_panels, and Network.ray_normals as a whole by the wall clock (it reads one count
            back); the median angle between the 'gradient' and the 'screen' normals where both exist
    loop    run_movement on a 512^2 synthetic subject with maps = depth, normal, shaded and diagnostics on, the exact
            MLP path, cfg.amd.maps_normals = 'screen' and 'gradient' alternating, each twice: ms per frame
    mesh    N = 64 and 128: hnrf_field_normals and Network.vertex_normals by device events; the median angle between
            the vertex normals and the area-weighted face normals of the extracted mesh
Recorded, not asserted: this is an opt-in diagnostic without a bound on time.  THE SEEDED NETWORK IS A NOISE FIELD: nothing
here has been looked at on a trained avatar."""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = (('frame', 400), ('loop', 700), ('mesh', 300))


def _net(dev):
    import torch
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state, with_density
    net = Network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0).items()})
    return net.to(dev).eval()


def _events(fn, reps=5):
    import torch
    fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)


FMT = lambda ms: '%.3f (%.3f .. %.3f)' % (ms[len(ms) // 2], ms[0], ms[-1])


def step_frame():
    import numpy as np, torch
    from humannerf_amd import geometry, ops, scene
    from humannerf_amd.config import cfg
    dev = torch.device('cuda:0')
    net = _net(dev)
    cfg.perturb, cfg.N_samples, cfg.amd.diagnostics = 0., 128, True
    size = 512
    fr = scene.synthetic_frame(H=size, W=size, pose_seed=3, pose_scale=0.3)
    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec', 'cnl_bbox_min_xyz',
            'cnl_bbox_scale_xyz', 'bgcolor']
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in keys}
    ray_index = torch.nonzero(torch.from_numpy(fr['ray_mask'].reshape(-1)).to(dev)).reshape(-1)
    with torch.no_grad():
        res = net(**data, iter_val=1e7)
        normal, nvalid, parts = net.ray_normals(data, res, want_parts=True)
    N, S = res['weights_on_rays'].shape
    n = parts['n']
    print('bench frame: %d rays of %d samples = %d samples; kept at weight_min = 1e-4: %d = %.2f %%; rays with a normal: %d'
          % (N, S, N * S, n, 100.0 * n / (N * S), int(nvalid.sum())))
    w = res['weights_on_rays'].contiguous()
    t_c = _events(lambda: ops.compact_samples(w, 1e-4))
    _, cond, _, hann_w, _ = net._conditioning(data['dst_posevec'].float(), 1e7, dev, True, want_rvec=False)
    with torch.no_grad():
        nr_packed = net._nonrigid_packed(cond)
        t_g = _events(lambda: net._density_gradient(None, (parts['x'], hann_w, nr_packed)))
        t_gc = _events(lambda: net._density_gradient(parts['x']))
        from humannerf_amd.network import motion_basis
        rvec = net.pose_decoder.rvec(data['dst_posevec'].float()[None]) if net._refines_pose(1e7) else None
        Rs, _ = motion_basis(data['dst_Rs'].float(), data['dst_Ts'].float(), data['cnl_gtfms'].float(), rvec)
        Rs = Rs.contiguous()
        bmw, alpha = res['backward_motion_weights'].contiguous(), res['alpha'].contiguous()
        t_r = _events(lambda: ops.ray_normals(w, bmw, Rs, parts['idx'], parts['count'], parts['g'], alpha, workspace=net._normals_ws))
        gm_s = geometry.frame_maps(data, res, size, size, ray_index, maps=['normal', 'shaded'])
        n_screen, v_screen = gm_s['normal_world'].clone(), gm_s['nvalid'].clone()
        t_screen = _events(lambda: geometry.frame_maps(data, res, size, size, ray_index, maps=['depth', 'normal', 'shaded']))
        t_grad = _events(lambda: geometry.frame_maps(data, res, size, size, ray_index, maps=['depth', 'normal', 'shaded'],
                                                     ray_normals=(normal, nvalid)))
        gm_g = geometry.frame_maps(data, res, size, size, ray_index, maps=['normal', 'shaded'], ray_normals=(normal, nvalid))
        wall = []
        for _ in range(5):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            net.ray_normals(data, res)
            torch.cuda.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
    print('device events, 5 repeats, median (min .. max), ms per call:')
    print('  hnrf_compact_samples over the weights %s' % FMT(t_c))
    print('  gradient pass over the %d kept samples, non-rigid chain included %s  (canonical chain alone %s); chunks of %d, '
          'workspace %d bytes per sample' % (n, FMT(t_g), FMT(t_gc), ops.GRADIENT_CHUNK,
                                             ops.GRADIENT_BYTES_CANONICAL + ops.GRADIENT_BYTES_NONRIGID))
    print('  hnrf_ray_normals (memset + 2 launches) %s' % FMT(t_r))
    print('  frame_maps, depth + normal + shaded: screen %s | with ray normals (hnrf_normal_panels in the place of the '
          'normals of hnrf_geometry_maps) %s' % (FMT(t_screen), FMT(t_grad)))
    print('  Network.ray_normals as a whole, wall clock with its one read-back: %s' % FMT(sorted(wall)))
    both = (gm_g['nvalid'] > 0) & (v_screen > 0)
    a, b = gm_g['normal_world'][both].double(), n_screen[both].double()
    ang = torch.rad2deg(torch.atan2(torch.linalg.cross(a, b).norm(dim=-1), (a * b).sum(-1)))
    flipped = torch.minimum(ang, 180 - ang)
    print("'gradient' against 'screen' normals on the %d pixels where both exist: median angle %.1f deg (%.1f deg up to sign: "
          "the screen normals are flipped towards the camera, the gradient normals are not).  Recorded, not asserted: the "
          'seeded network is a noise field.' % (int(both.sum()), float(ang.median()), float(flipped.median())), flush=True)


def step_loop(n):
    import numpy as np, torch
    from humannerf_amd import dataset, render, run, scene
    from humannerf_amd.config import cfg
    d = tempfile.mkdtemp()
    scene.write_synthetic_subject(d, n_frames=n, size=512, binary_mask=True)
    cfg.resize_img_scale = 1.0
    cfg.N_samples, cfg.perturb, cfg.amd.diagnostics, cfg.amd.loop_timing = 128, 0., True, True
    cfg.amd.metrics, cfg.amd.video, cfg.amd.maps = 'device', 'mjpeg_only', ['depth', 'normal', 'shaded']
    dev = torch.device('cuda:0')
    subj = dataset.Subject(d)
    net = _net(dev)
    out = tempfile.mkdtemp()

    def one(tag, how, frames):
        cfg.amd.maps_normals = how
        torch.cuda.synchronize(); t0 = time.perf_counter()
        run.run_movement(net, subj, render_folder_name=tag, logdir=out, device=dev, test_num=frames, metrics=[])
        torch.cuda.synchronize()
        lp = render.render_frames.last_prefetch
        return (time.perf_counter() - t0) * 1e3 / frames, float(np.median(lp['gpu_ms']))

    for how in ('screen', 'gradient'):
        one('warm_' + how, how, 3)
    res = {'screen': [], 'gradient': []}
    for rep in range(2):
        for how in ('screen', 'gradient'):
            res[how].append(one('t%d_%s' % (rep, how), how, n))
    print('run_movement, %d frames of 512 x 512 x 128, exact MLP path, diagnostics on, maps depth + normal + shaded, video '
          'mjpeg_only; ms per frame by the wall clock | gpu busy per frame (median of the frames\' events), two repeats each, '
          'alternating:' % n)
    for how in ('screen', 'gradient'):
        a, b = res[how]
        print("  maps_normals = %-10r %8.2f | %8.2f   and   %8.2f | %8.2f" % (how, a[0], a[1], b[0], b[1]))
    s, g = res['screen'], res['gradient']
    print("  'gradient' - 'screen': %+.2f ms per frame by the wall clock (means of two), %+.2f ms gpu busy; spread of the two "
          "'screen' repeats %.2f ms.  No acceptance bound: an opt-in diagnostic."
          % (0.5 * (g[0][0] + g[1][0] - s[0][0] - s[1][0]), 0.5 * (g[0][1] + g[1][1] - s[0][1] - s[1][1]), abs(s[0][0] - s[1][0])),
          flush=True)


def step_mesh():
    import numpy as np, torch
    from humannerf_amd import ops, scene
    dev = torch.device('cuda:0')
    net = _net(dev)
    cam = scene.synthetic_frame(H=64, W=64, camera_only=True)
    priors = torch.from_numpy(cam['motion_weights_priors']).to(dev)
    bmin, bmax = cam['cnl_bbox_min_xyz'], cam['cnl_bbox_max_xyz']
    for N in (64, 128):
        with torch.no_grad():
            verts, faces, _ = net.extract_canonical_mesh(bmin, bmax, priors, resolution=N, level=10.0)
            vn, g, sigma, vol = net.vertex_normals(verts, priors, bmin, bmax, want_parts=True)
            b0, _, sc = net._mesh_bbox(bmin, bmax)
            t_f = _events(lambda: ops.field_normals(verts, g, sigma, vol, vol.shape[0] - 1, b0, sc))
            t_v = _events(lambda: net.vertex_normals(verts, priors, bmin, bmax))
        f = faces.long()
        p0, p1, p2 = (verts[f[:, k]].double() for k in range(3))
        fn = torch.linalg.cross(p1 - p0, p2 - p0)                             # length = twice the area
        acc = torch.zeros(verts.shape[0], 3, dtype=torch.float64, device=dev)
        for k in range(3):
            acc.index_add_(0, f[:, k], fn)
        ok = (acc.norm(dim=1) > 0) & (vn.norm(dim=1) > 0)
        a, b = vn[ok].double(), acc[ok] / acc[ok].norm(dim=1, keepdim=True)
        ang = torch.rad2deg(torch.atan2(torch.linalg.cross(a, b).norm(dim=-1), (a * b).sum(-1)))
        print('N = %3d: %d vertices, %d faces; hnrf_field_normals %s ms; Network.vertex_normals (gradient pass included) %s ms; '
              'median angle between the vertex normals and the area-weighted face normals %.1f deg (%.1f deg up to sign; the '
              'winding of the marching tetrahedra is not what is compared), %d vertices with both'
              % (N, verts.shape[0], faces.shape[0], FMT(t_f), FMT(t_v), float(ang.median()),
                 float(torch.minimum(ang, 180 - ang).median()), int(ok.sum())), flush=True)
    print('Recorded, not asserted.  The seeded network is a noise field: nothing was looked at on a trained avatar.')


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    if len(sys.argv) > 2 and sys.argv[1] == '--step':
        n = int(sys.argv[3]) if len(sys.argv) > 3 else 12
        {'frame': step_frame, 'loop': lambda: step_loop(n), 'mesh': step_mesh}[sys.argv[2]]()
        sys.exit(0)
    n = sys.argv[1] if len(sys.argv) > 1 else '12'
    head = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip()
    print('python profiles/tools/time_normals.py %s   (on top of commit %s; one MI355X, profiler off)' % (n, head or '?'), flush=True)
    for step, limit in STEPS:
        print('---- %s' % step, flush=True)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, n], timeout=limit, cwd=ROOT).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print('step %s ended with status %d: stopping' % (step, rc), flush=True)
            sys.exit(rc if rc > 0 else 1)
