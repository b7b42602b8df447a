"""What the heads of a multi-head canonical MLP cost, from HIP events with the profiler off.  One JSON line per step:

  kernel  K3 on 4 194 304 samples (one ray chunk of 32 768 x 128): the all-heads launch (hnrf_canonical_heads_fwd,
          H = --heads) against the single-head launch (hnrf_canonical_fwd) of this build and -- with --parent-lib, a
          libhnrf.so built from the parent commit -- of the parent, interleaved in the same process on the same inputs;
          both arithmetics.  Accepted: all-heads / parent single-head <= 1.05 (f16x3).
  frame   the bench frame (512 x 512 rays x 128 samples, bench.py's camera): forward(head_id=-1) against the H frames
          forward(head_id=h), with cfg.amd.share_underflow on and off (when profiles/multihead.txt was taken the
          all-heads path bypassed the shared evaluation either way; since then it shares:
          time_multihead_shared.py), 11-output and lean form.

    python profiles/tools/time_multihead.py [--heads 4] [--iters 20] [--warmup 3] [--parent-lib PATH] [--step kernel|frame]

Every step stands alone: the caller runs one step per process under its own timeout, chained so that a failure ends the
run; without --step both run in this process.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from humannerf_amd import _lib, ops, scene  # noqa: E402
from humannerf_amd.config import cfg  # noqa: E402
from humannerf_amd.seeded import default_shapes, seeded_state  # noqa: E402

P_KERNEL = 32768 * 128
W_KEY, B_KEY = 'cnl_mlp.module.output_linear.0.weight', 'cnl_mlp.module.output_linear.0.bias'


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


def head_state(state, H, seed=3):
    """``state`` with H heads: head 0 is the seeded single head, the others are copies of it with seeded noise."""
    rs = np.random.RandomState(seed)
    W, b = state[W_KEY], state[B_KEY]
    st = dict(state)
    st[W_KEY] = np.concatenate([W] + [W * rs.uniform(0.8, 1.2, W.shape).astype(np.float32) for _ in range(H - 1)])
    st[B_KEY] = np.concatenate([b] * H)
    return st


def layers(st, dev):
    idx = [0, 2, 4, 6, 8, 10, 12, 14]
    T = lambda a: torch.from_numpy(a).to(dev)
    return ([T(st[f'cnl_mlp.module.pts_linears.{i}.weight']) for i in idx] + [T(st[W_KEY])],
            [T(st[f'cnl_mlp.module.pts_linears.{i}.bias']) for i in idx] + [T(st[B_KEY])])


def step_kernel(args, state, dev):
    H = args.heads
    xyz = torch.from_numpy(np.random.RandomState(1).uniform(-1.0, 1.0, (P_KERNEL, 3)).astype(np.float32)).to(dev)
    w1, b1 = layers(state, dev)
    wh, bh = layers(head_state(state, H), dev)
    parent = None
    if args.parent_lib:
        _lib.load()                                            # (torch's HIP runtime first, as _lib.load arranges)
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.hnrf_canonical_packed_bytes.restype = ctypes.c_size_t
    res = {'step': 'kernel', 'samples': P_KERNEL, 'heads': H, 'parent_lib': bool(parent)}
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for mode in ('f16x3', 'f32'):
        m = ops.MLP_MODES[mode]
        one = ops.canonical_pack(w1, b1, mode)
        every = ops.canonical_heads_pack(wh, bh, H, mode)
        raw1 = torch.empty(P_KERNEL, 4, device=dev)
        rawh = torch.empty(H, P_KERNEL, 4, device=dev)
        lib = _lib.load_heads()
        fns = {'single': lambda: lib.hnrf_canonical_fwd(xyz.data_ptr(), one.data_ptr(), m, P_KERNEL, raw1.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream),
               'heads': lambda: lib.hnrf_canonical_heads_fwd(xyz.data_ptr(), every.data_ptr(), m, P_KERNEL, H, rawh.data_ptr(),
                                                             torch.cuda.current_stream().cuda_stream)}
        if parent is not None:
            pp = torch.empty(parent.hnrf_canonical_packed_bytes(m) // 4 + 64, device=dev)
            vp = lambda t: ctypes.c_void_p(t.data_ptr())
            rc = parent.hnrf_canonical_pack(ops._ptr_array(w1), ops._ptr_array(b1), m, vp(pp), stream())
            assert rc == 0, rc
            rawp = torch.empty(P_KERNEL, 4, device=dev)
            fns['parent_single'] = lambda: parent.hnrf_canonical_fwd(vp(xyz), vp(pp), m, ctypes.c_int64(P_KERNEL), vp(rawp),
                                                                     stream())
        t = interleaved_ms(fns, args.iters, args.warmup)
        torch.cuda.synchronize()
        t['head0_equals_single'] = bool(torch.equal(rawh[0], raw1))
        if parent is not None:
            t['parent_equals_single'] = bool(torch.equal(rawp, raw1))
            t['heads_over_parent_single'] = round(t['heads']['median'] / t['parent_single']['median'], 4)
        t['heads_over_single'] = round(t['heads']['median'] / t['single']['median'], 4)
        res[mode] = t
    print(json.dumps(res), flush=True)


def step_frame(args, state, dev):
    from humannerf_amd.network import Network
    H = args.heads
    cfg.canonical_mlp.multihead = {'enable': True, 'head_depth': 1}
    cfg.multihead = {'head_num': H}
    net = Network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in head_state(state, H).items()}, strict=True)
    net = net.to(dev).eval()
    cfg.perturb, cfg.N_samples, cfg.ignore_non_rigid_motions = 0., 128, False
    fr = scene.synthetic_frame(H=512, W=512, focal_at_512=1700.0, pose_seed=0)
    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
            'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in keys}
    res = {'step': 'frame', 'heads': H, 'rays': int(data['rays'].shape[1]), 'samples': 128, 'chunk': int(cfg.chunk)}

    def each():
        for h in range(H):
            net(**data, head_id=h, iter_val=1e7)

    with torch.no_grad():
        for diag in (True, False):
            cfg.amd.diagnostics = diag
            t = {}
            for share in (True, False):
                cfg.amd.share_underflow = share
                r = interleaved_ms({'all_heads': lambda: net(**data, head_id=-1, iter_val=1e7), 'each_head': each},
                                   args.iters, args.warmup)
                r['all_over_each'] = round(r['all_heads']['median'] / r['each_head']['median'], 4)
                r['all_over_one_frame'] = round(r['all_heads']['median'] / (r['each_head']['median'] / H), 4)
                t['share_on' if share else 'share_off'] = r
            res['11-output' if diag else 'lean'] = t
        net.check_f16_range(wait=True)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--heads', type=int, default=4)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--step', choices=['kernel', 'frame'], default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    state = seeded_state(default_shapes(), seed=0)
    if args.step in (None, 'kernel'):
        step_kernel(args, state, dev)
    if args.step in (None, 'frame'):
        step_frame(args, state, dev)


if __name__ == '__main__':
    main()
