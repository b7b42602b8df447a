"""What the geometry maps cost and how they agree with the mesh preview (cfg.amd.maps, humannerf_amd/geometry.py,
csrc/hnrf_geometry.hip).
    python profiles/tools/time_geometry.py [n_frames] [--parent <built checkout of the parent commit>] > profiles/geometry_maps.txt
The driver starts every step as a child process of its own under a time limit and stops at the first that fails:
    twin    no GPU: the accuracy of the screen-space normals on the analytic scenes of tests/test_geometry_refs.py
    op      the three library calls alone by device events, 5 x 200 calls on a 512 x 512 frame with a ray per pixel:
            (a) lean inputs, depth + normal + shaded; (b) diagnostics inputs (S = 128), all four panels, both surfaces
    loop    run_movement on a 512^2 synthetic subject with cfg.amd.canonical = cfg.amd.nonrigid = 'baked' and
            video = 'mjpeg_only', maps off and on ('depth', 'normal', 'shaded'), alternating, each twice; with --parent
            the same loop (maps off: it has no such option) from the parent's tree before and after, in the same job
    mesh    the frame and the seeded network of profiles/tools/time_mesh_render.py: the median angle between the maps'
            normals and the rasteriser's shade = 'normal' picture where both cover, and the median |t - mesh depth| for
            both surfaces (recorded, not asserted: nothing derives them)
Nothing here has been looked at on a trained avatar: the network is the seeded one."""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = (('twin', 120), ('op', 240), ('loop', 600), ('mesh', 300))


def step_twin():
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import geometry_cases as gc
    from humannerf_amd import geometry as geo
    for n in gc.PLANES:
        H, W = 17, 33
        o, d, surf, p2r = gc.full_frame(H, W, gc.plane_t(n, 0.0, H, W))
        res = geo.maps_host(o, d, surf, p2r, H, W, want=('normal', 'nvalid'), edge=1e9, bgcolor=(0, 0, 0))
        d64 = gc.camera(H, W)[1].reshape(H, W, 3)
        nn = np.asarray(n, np.float64) / np.linalg.norm(n)
        truth = np.where(((d64 * nn).sum(-1) > 0)[..., None], -nn, nn)
        ang = gc.angle_deg(res['normal'], truth)
        print('plane n = %-18r 17 x 33: normals on %d of %d pixels; angle to the plane normal: interior max %.2e deg, '
              'whole image max %.2e deg' % (n, res['nvalid'].sum(), H * W, ang[1:-1, 1:-1].max(), ang.max()))
    H = W = 32
    t64, hit = gc.sphere_t(0.5, H, W)
    o, d, surf, p2r = gc.full_frame(H, W, t64, hit)
    res = geo.maps_host(o, d, surf, p2r, H, W, want=('normal', 'nvalid'), edge=0.05, bgcolor=(0, 0, 0))
    o64, d64 = gc.camera(H, W)
    P = o64 + d64 * t64[:, None]
    nt = P / np.linalg.norm(P, axis=1, keepdims=True)
    sel = (hit & (-(nt * d64).sum(1) / np.linalg.norm(d64, axis=1) > 0.5)).reshape(H, W)
    err = gc.angle_deg(res['normal'], nt.reshape(H, W, 3))[sel]
    print('sphere r = 0.5, 32 x 32, edge 0.05: %d pixels with -n.d > 0.5, %d of them with a normal, error max %.3f deg, mean '
          '%.3f deg' % (sel.sum(), res['nvalid'][sel].sum(), err.max(), err.mean()), flush=True)


def _events(fn, reps=5, calls=200):
    import torch
    for _ in range(20):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(1e3 * e0.elapsed_time(e1) / calls)
    return sorted(ms)


def step_op():
    import numpy as np, torch
    from humannerf_amd import ops
    dev = torch.device('cuda:0')
    H = W = 512
    N, S = H * W, 128
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing='ij')
    d = torch.stack([(xs - W / 2) / 1250., (ys - H / 2) / 1250., -torch.ones(H, W, device=dev)], -1).reshape(N, 3).contiguous()
    o = torch.tensor([0., 0., 3.], device=dev).repeat(N, 1)
    blob = (((xs - 256) / 120.) ** 2 + ((ys - 256) / 220.) ** 2 < 1).reshape(N)                # a body-sized silhouette
    alpha = torch.where(blob, 0.6 + 0.4 * rnd(N), 0.3 * rnd(N))
    depth = alpha * (3.0 - 0.3 * torch.cos((xs.reshape(N) - 256) / 120.))
    near, far = torch.full((N,), 2.4, device=dev), torch.full((N,), 3.6, device=dev)
    w = rnd(N, S) ** 8
    w = w / w.sum(1, keepdim=True) * alpha[:, None]
    off = 0.01 * (rnd(N, S, 3) - 0.5)
    ray_index = torch.arange(N, device=dev)
    truth8 = (255 * rnd(H, W, 3)).to(torch.uint8)
    M, bg, lohi = torch.eye(3, device=dev), torch.zeros(3, device=dev), torch.tensor([2.4, 3.6], device=dev)
    ws = {'t_exp': torch.empty(N, device=dev), 't_med': torch.empty(N, device=dev), 'woff': torch.empty(N, 3, device=dev),
          'valid': torch.empty(N, dtype=torch.uint8, device=dev)}
    pix, st = ops.pixel_rays(ray_index, H, W)
    panels = {k: torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for k in ('normal8', 'depth8', 'shaded8', 'offset8')}
    panels.update(normal=torch.empty(H, W, 3, device=dev), nvalid=torch.empty(H, W, dtype=torch.uint8, device=dev))
    print('512 x 512 frame, one ray per pixel (N = 262144), %.0f %% of the rays a surface; device events over 5 x 200 calls, '
          'median (min .. max), us per call' % (100 * float(blob.float().mean())))
    fmt = lambda ms: '%.1f (%.1f .. %.1f)' % (ms[len(ms) // 2], ms[0], ms[-1])
    for tag, kw, want, surface in (
            ('(a) lean inputs, depth + normal + shaded', {}, ['normal', 'nvalid', 'depth8', 'normal8', 'shaded8'], 0),
            ('(b) diagnostics inputs S = 128, all four panels, expected surface', dict(want_median=False, want_woff=True),
             ['normal', 'nvalid', 'depth8', 'normal8', 'shaded8', 'offset8'], 0),
            ('(b) diagnostics inputs S = 128, all four panels, median surface', dict(want_median=True, want_woff=True),
             ['normal', 'nvalid', 'depth8', 'normal8', 'shaded8', 'offset8'], 1)):
        diag = bool(kw)
        surf_fn = lambda: ops.ray_surface(near, far, alpha, depth, w if diag else None, off if diag else None, out=ws, **kw)
        surf = surf_fn()
        maps_fn = lambda: ops.geometry_maps(o, d, surf, pix, H, W, want, surface=surface, alpha=alpha, M=M, bgcolor=bg, lohi=lohi,
                                            truth8=truth8 if diag else None, status=st, out=panels)
        a, b, c = _events(surf_fn), _events(lambda: ops.pixel_rays(ray_index, H, W, pix2ray=pix, status=st)), _events(maps_fn)
        tot = _events(lambda: (surf_fn(), ops.pixel_rays(ray_index, H, W, pix2ray=pix, status=st), maps_fn()))
        res = maps_fn()
        torch.cuda.synchronize()
        print('  %s\n      hnrf_ray_surface %s | hnrf_pixel_rays (3 launches + a memset) %s | hnrf_geometry_maps %s | the three '
              'back to back %s; sum of the medians %.1f; normals on %d pixels; HBM bytes read by hnrf_ray_surface %.0f MB'
              % (tag, fmt(a), fmt(b), fmt(c), fmt(tot), a[2] + b[2] + c[2], int(res['nvalid'].sum()),
                 (N * S * 16 * (2 if kw.get('want_median') else 1) if diag else N * 8) / 1e6), flush=True)


def step_loop(n, parent):
    root = parent or ROOT
    sys.path.insert(0, root)
    import numpy as np, torch
    from humannerf_amd import dataset, render, run, scene
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state, with_density
    assert os.path.abspath(os.path.dirname(os.path.dirname(run.__file__))) == os.path.abspath(root)
    d = tempfile.mkdtemp()
    scene.write_synthetic_subject(d, n_frames=n, size=512, binary_mask=True)
    cfg.resize_img_scale = 1.0
    cfg.N_samples, cfg.perturb, cfg.amd.diagnostics, cfg.amd.loop_timing = 128, 0., False, True
    cfg.amd.canonical, cfg.amd.nonrigid, cfg.amd.metrics, cfg.amd.video = 'baked', 'baked', 'device', 'mjpeg_only'
    dev = torch.device('cuda:0')
    subj = dataset.Subject(d)
    net = Network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in with_density(seeded_state(default_shapes(), 0), bias_delta=5.0).items()})
    net = net.to(dev).eval()
    out = tempfile.mkdtemp()
    ways = [('maps off', [])] + ([] if parent else [('maps on', ['depth', 'normal', 'shaded'])])

    def one(tag, maps, frames):
        if not parent:
            cfg.amd.maps = maps
        torch.cuda.synchronize(); t0 = time.perf_counter()
        run.run_movement(net, subj, render_folder_name=tag, logdir=out, device=dev, test_num=frames, metrics=[])
        torch.cuda.synchronize()
        lp = render.render_frames.last_prefetch
        return (time.perf_counter() - t0) * 1e3 / frames, float(np.median(lp['gpu_ms'])), float(np.median(lp['gpu_gap_ms']))

    for k, (_, maps) in enumerate(ways):
        one('warm_%d' % k, maps, 4)
    res = {w[0]: [] for w in ways}
    for rep in range(2):
        for k, (name, maps) in enumerate(ways):
            res[name].append(one('t%d_%d' % (rep, k), maps, n))
    who = 'parent commit' if parent else 'this commit'
    for name, _ in ways:
        a, b = res[name]
        print('  %-13s %-9s %7.3f | %7.3f ms per frame by the wall clock (spread %.3f); gpu busy per frame %.3f | %.3f ms, gpu '
              'gap %.3f | %.3f ms (medians of the frames\' events)' % (who, name, a[0], b[0], abs(a[0] - b[0]), a[1], b[1], a[2], b[2]),
              flush=True)
    if not parent:
        off, on = res['maps off'], res['maps on']
        print('  maps on - maps off: wall clock %+.3f ms per frame (means of two), gpu busy %+.3f ms per frame; spread of the two '
              'maps-off repeats %.3f ms.  Accepted when the added time is no more than that spread plus the sum of the three '
              'kernel times of step op (a)' % (0.5 * (on[0][0] + on[1][0] - off[0][0] - off[1][0]),
                                                0.5 * (on[0][1] + on[1][1] - off[0][1] - off[1][1]), abs(off[0][0] - off[1][0])),
              flush=True)


def step_mesh():
    sys.path.insert(0, ROOT)
    import numpy as np, torch
    from humannerf_amd import geometry, scene
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state, with_density
    dev = torch.device('cuda:0')
    net = Network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0).items()})
    net = net.to(dev).eval()
    cfg.perturb, cfg.N_samples, cfg.amd.diagnostics = 0., 128, True
    size, N = 512, 256
    cam = scene.synthetic_frame(H=size, W=size, pose_seed=3, pose_scale=0.3, camera_only=True)
    priors = torch.from_numpy(cam['motion_weights_priors']).to(dev)
    cam['motion_weights_priors'] = priors
    fr = scene.synthetic_frame(H=size, W=size, pose_seed=3, pose_scale=0.3)
    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'dst_posevec', 'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in keys}
    data['motion_weights_priors'] = priors
    ray_index = torch.nonzero(torch.from_numpy(fr['ray_mask'].reshape(-1)).to(dev)).reshape(-1)
    E = np.asarray(cam['E'], np.float32)[:3, :3]
    with torch.no_grad():
        verts, faces, colors = net.extract_canonical_mesh(cam['cnl_bbox_min_xyz'], cam['cnl_bbox_max_xyz'], priors, resolution=N, level=10.0)
        mesh = net.render_mesh(verts, faces, colors, cam, cull='back', shade='normal')
        res = net(**data, iter_val=1e7)
    covered = mesh['alpha'] > 0.5
    n_mesh = mesh['rgb'] * 2 - 1                                           # camera frame: 0.5 + 0.5 (E n)
    line = []
    for surface in geometry.SURFACES:
        gm = geometry.frame_maps(data, res, size, size, ray_index, maps=['normal'], surface=surface, M=E)
        n_cam = gm['normal_world'] @ torch.from_numpy(E).to(dev).T
        both = covered & (gm['nvalid'] > 0)
        a, b = n_cam[both].double(), n_mesh[both].double()
        ang = torch.rad2deg(torch.atan2(torch.linalg.cross(a, b).norm(dim=-1), (a * b).sum(-1)))
        t_img = torch.zeros(size * size, device=dev).index_copy_(0, ray_index, gm['t']).reshape(size, size)
        v_img = torch.zeros(size * size, dtype=torch.uint8, device=dev).index_copy_(
            0, ray_index, ((gm['t'] != 0)).to(torch.uint8)).reshape(size, size) > 0
        sel = covered & v_img
        line.append('%s surface: normals on %d pixels, %d of them under the mesh, median angle to the mesh normal %.2f deg; median '
                    '|t - mesh depth| %.5f over %d pixels' % (surface, int((gm['nvalid'] > 0).sum()), int(both.sum()),
                                                              float(ang.median()), float((t_img - mesh['depth'])[sel].abs().median()),
                                                              int(sel.sum())))
    print('mesh preview (seeded network, sigma bias + 5, level 10, N = %d, 512 x 512, pose seed 3; %d pixels covered) against the '
          'geometry maps of the volume render of the same frame:' % (N, int(covered.sum())))
    for l in line:
        print('  ' + l, flush=True)


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    if len(sys.argv) > 2 and sys.argv[1] == '--step':
        n = int(sys.argv[3]) if len(sys.argv) > 3 else 200
        parent = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] else None
        if sys.argv[2] == 'loop' and parent:
            sys.path.remove(ROOT)
        {'twin': step_twin, 'op': step_op, 'loop': lambda: step_loop(n, parent), 'mesh': step_mesh}[sys.argv[2]]()
        sys.exit(0)
    args = [a for a in sys.argv[1:]]
    parent = ''
    if '--parent' in args:
        parent = os.path.abspath(args[args.index('--parent') + 1])
        del args[args.index('--parent'):args.index('--parent') + 2]
    n = args[0] if args else '200'
    head = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip()
    print('python profiles/tools/time_geometry.py %s%s   (on top of commit %s; one MI355X, profiler off)'
          % (n, ' --parent <parent checkout>' if parent else '', head or '?'), flush=True)
    plan = []
    for step, limit in STEPS:
        if step == 'loop' and parent:
            plan += [('loop', limit, parent), ('loop', limit, ''), ('loop', limit, parent)]
        else:
            plan.append((step, limit, ''))
    for step, limit, par in plan:
        print('---- %s%s' % (step, ' (parent commit)' if par else ''), flush=True)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, n, par], timeout=limit,
                                cwd=par or ROOT).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print('step %s ended with status %d: stopping' % (step, rc), flush=True)
            sys.exit(rc if rc > 0 else 1)
