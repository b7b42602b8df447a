"""What view-dependent colour (canonical_mlp.view_dir with cfg.amd.view_dir) costs, from HIP events with the profiler
off.  One JSON line per step:

  frame    the bench frame (512 x 512 rays x 128 samples, bench.py's camera), lean form: a view-dependent network
           against the view-independent one of the same library, in turns in the same process, with the exact renderer
           (cfg.amd.canonical = 'mlp', share_underflow as configured) and the baked one ('baked'); with --parent-lib, a
           libhnrf.so built from the parent commit, also the view-independent frame with every library call routed to
           it.  Expected from the code: one more launch over 262 144 rays and 12 more bytes per ray read in K4.
  kernels  hnrf_view_bias_fwd on 262 144 rays; on the training shape, 6 144 rays x 128: hnrf_composite_view_bwd (with
           d_bias) against hnrf_composite_bwd, and hnrf_view_bias_bwd.
  train    one optimizer step (Trainer.train_step, MSE objective, steady-state iteration) on 6 144 rays x 128 with and
           without view colour, in turns.

    python profiles/tools/time_view_dir.py [--iters 20] [--warmup 3] [--parent-lib PATH] [--step frame|kernels|train]

Every step stands alone: the caller runs one step per process under its own timeout, chained so that a failure ends the
run; without --step all run in this process.  The weights are the seeded ones; the view layers keep their default
initialisation except the density layer, which is the seeded head's sigma row (so both networks render the same
densities).  Nothing here says anything about picture quality."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from humannerf_amd import _lib, ops, scene  # noqa: E402
from humannerf_amd.config import cfg  # noqa: E402
from humannerf_amd.seeded import default_shapes, seeded_state  # noqa: E402

KEYS = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec', 'cnl_bbox_min_xyz',
        'cnl_bbox_scale_xyz', 'bgcolor']
W_KEY, B_KEY = 'cnl_mlp.module.output_linear.0.weight', 'cnl_mlp.module.output_linear.0.bias'
BANDS = 4


def spread(ms):
    ms = sorted(ms)
    return {'median': round(ms[len(ms) // 2], 4), 'min': round(ms[0], 4), 'max': round(ms[-1], 4), 'n': len(ms)}


def interleaved_ms(fns, iters, warmup):
    """Event times of every callable of ``fns``, taken in turns (a, b, c, a, b, c, ...): clock drift hits all alike."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    ev = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    return {k: spread([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}


def networks(dev, train=False):
    """(view-independent network, view-dependent network) on the seeded state; cfg is left with view colour ON (the
    options are read per call only by a network that has the branch)."""
    from humannerf_amd.network import Network
    state = seeded_state(default_shapes(), seed=0)
    plain = Network()
    plain.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    cfg.canonical_mlp.view_dir, cfg.canonical_mlp.view_embed, cfg.canonical_mlp.multires_dir = True, 'mlp', BANDS
    cfg.canonical_mlp.view_dir_camera_only = False
    cfg.amd.view_dir = True
    torch.manual_seed(0)
    view = Network()
    rest = {k: torch.from_numpy(v) for k, v in state.items() if '.output_linear.' not in k}
    missing = view.load_state_dict(rest, strict=False)
    assert all('output_linear_' in k for k in missing.missing_keys) and not missing.unexpected_keys
    with torch.no_grad():
        view.cnl_mlp.module.output_linear_density[0].weight.copy_(torch.from_numpy(state[W_KEY][3:4]))
        view.cnl_mlp.module.output_linear_density[0].bias.copy_(torch.from_numpy(state[B_KEY][3:4]))
    view.weights_changed()
    nets = [n.to(dev) for n in (plain, view)]
    return [n.train() if train else n.eval() for n in nets]


def parent_library(path):
    _lib.load()                                                # (torch's HIP runtime first, as _lib.load arranges)
    parent = ctypes.CDLL(os.path.abspath(path))
    for name, (res, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(parent, name)
        fn.restype, fn.argtypes = res, argtypes
    return parent


def routed(fn, parent, own):
    def call():
        _lib._lib = parent
        try:
            return fn()
        finally:
            _lib._lib = own
    return call


def step_frame(args, dev):
    plain, view = networks(dev)
    cfg.perturb, cfg.N_samples, cfg.ignore_non_rigid_motions = 0., 128, False
    cfg.amd.diagnostics = False
    fr = scene.synthetic_frame(H=512, W=512, focal_at_512=1700.0, pose_seed=0)
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in KEYS}
    data['cnl_bbox_max_xyz'] = torch.from_numpy(np.ascontiguousarray(fr['cnl_bbox_max_xyz'])).to(dev)
    res = {'step': 'frame', 'rays': int(data['rays'].shape[1]), 'samples': 128, 'chunk': int(cfg.chunk),
           'share_underflow': bool(cfg.amd.share_underflow), 'parent_lib': bool(args.parent_lib)}
    own = _lib.load_open()
    parent = parent_library(args.parent_lib) if args.parent_lib else None
    with torch.no_grad():
        for canonical in ('mlp', 'baked'):
            cfg.amd.canonical = canonical
            fns = {'plain': lambda: plain(**data, iter_val=1e7), 'view': lambda: view(**data, iter_val=1e7)}
            if parent is not None:
                fns['plain_parent_lib'] = routed(fns['plain'], parent, own)
            t = interleaved_ms(fns, args.iters, args.warmup)
            t['view_over_plain'] = round(t['view']['median'] / t['plain']['median'], 4)
            t['plain_spread'] = round((t['plain']['max'] - t['plain']['min']) / t['plain']['median'], 4)
            if parent is not None:
                t['plain_over_parent'] = round(t['plain']['median'] / t['plain_parent_lib']['median'], 4)
            res[canonical] = t
        cfg.amd.canonical = 'mlp'
        plain.check_f16_range(wait=True)
        view.check_f16_range(wait=True)
    print(json.dumps(res), flush=True)


def step_kernels(args, dev):
    lib = _lib.load_view()
    rs = np.random.RandomState(0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).to(dev)
    E = 3 + 6 * BANDS
    N = 512 * 512
    dirs, B, c = T(rs.standard_normal((N, 3))), T(rs.uniform(-1, 1, (3, E))), T(rs.uniform(-1, 1, 3))
    res = {'step': 'kernels', 'bands': BANDS}
    res['view_bias_fwd_262144_rays'] = interleaved_ms({'ms': lambda: ops.view_bias(dirs, B, c)}, args.iters, args.warmup)['ms']
    R, S = 6144, 128
    raw, mask = T(rs.standard_normal((R, S, 4)) * 2), T(rs.uniform(0, 1.1, (R, S)))
    z, rays_d = T(np.sort(1 + rs.uniform(0, 3, (R, S)), axis=1)), T(rs.standard_normal((R, 3)))
    bg, g_rgb, bias = T(np.array([200., 100., 30.])), T(rs.standard_normal((R, 3))), T(rs.standard_normal((R, 3)))
    d_raw, d_mask, d_bias = torch.empty_like(raw), torch.empty_like(mask), torch.empty_like(bias)
    st = lambda: torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    t = interleaved_ms({
        'composite_bwd': lambda: lib.hnrf_composite_bwd(p(raw), p(mask), p(z), p(rays_d), p(bg), p(g_rgb), None, None, R, S,
                                                        p(d_raw), p(d_mask), st()),
        'composite_view_bwd': lambda: lib.hnrf_composite_view_bwd(p(raw), p(mask), p(z), p(rays_d), p(bg), p(bias), p(g_rgb),
                                                                  None, None, R, S, p(d_raw), p(d_mask), p(d_bias), st())},
        args.iters, args.warmup)
    res['composite_bwd_6144x128'] = t
    need = lib.hnrf_view_bias_bwd_workspace_bytes(R, BANDS)
    ws, dB, dc = torch.empty(need // 4 + 64, device=dev), torch.empty(3, E, device=dev), torch.empty(3, device=dev)
    res['view_bias_bwd_6144_rays'] = interleaved_ms(
        {'ms': lambda: lib.hnrf_view_bias_bwd(p(dirs), p(d_bias), BANDS, R, p(ws), need, p(dB), p(dc), st())},
        args.iters, args.warmup)['ms']
    print(json.dumps(res), flush=True)


def step_train(args, dev):
    from humannerf_amd.train import Trainer
    cfg.perturb, cfg.N_samples = 1.0, 128
    cfg.train.lossweights = {'lpips': 0.0, 'mse': 0.2, 'l1': 0.0}
    plain, view = networks(dev, train=True)
    fr = scene.synthetic_frame(H=512, W=512, focal_at_512=1700.0)
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in KEYS}
    idx = []
    for k in range(6):                                         # the bench's item: six 32 x 32 windows, flat rays with targets
        y0, x0 = 96 + 48 * k, 80 + 56 * k
        yy, xx = np.meshgrid(np.arange(y0, y0 + 32), np.arange(x0, x0 + 32), indexing='ij')
        idx.append((yy * 512 + xx).reshape(-1))
    idx = torch.from_numpy(np.concatenate(idx)).to(dev)
    tb = dict(data, rays=data['rays'][:, idx].contiguous(), near=data['near'][idx].contiguous(), far=data['far'][idx].contiguous())
    gen = torch.Generator(device=dev).manual_seed(1)
    tb['target_rgbs'] = torch.rand(6144, 3, device=dev, generator=gen)
    tb['t_rand'] = torch.rand(6144, 128, device=dev, generator=gen)
    trainers = {}
    for name, net in (('plain', plain), ('view', view)):
        trainers[name] = Trainer(net)
        trainers[name].iter = 60000
    t = interleaved_ms({k: (lambda tr=tr: tr.train_step(tb)) for k, tr in trainers.items()}, args.iters, args.warmup + 2)
    t['view_over_plain'] = round(t['view']['median'] / t['plain']['median'], 4)
    print(json.dumps(dict(step='train', rays=6144, samples=128, **t)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--step', choices=['frame', 'kernels', 'train'], default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for name, fn in (('frame', step_frame), ('kernels', step_kernels), ('train', step_train)):
        if args.step in (None, name):
            fn(args, dev)


if __name__ == '__main__':
    main()
