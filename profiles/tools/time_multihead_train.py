"""What training a multi-head canonical MLP costs (cfg.amd.train_heads), on the bench's training shape: 6 144 rays x 128
samples, one MI355X, steady-state iteration (past kick_in_iter / full_band_iter), MSE objective, H = --heads.

    python profiles/tools/time_multihead_train.py [--heads 4] [--steps 20] [--warmup 5] [--repeats 2] [--parent-lib PATH]

Ways of taking one optimizer step, each timed --repeats times in turns (HIP events around --steps back-to-back steps):
  single         the single-head network of this library (Trainer.train_step)
  parent_single  the same step with every library call routed to --parent-lib, a libhnrf.so built from the parent
                 commit, loaded next to this build's in the same process (no existing kernel instance was to change:
                 `single` is expected inside the spread of parent_single's own repeats; both ranges are printed)
  head           the multi-head network, head_id = 1: the single-head kernels on rows 4..7 of output_linear.0
  all_heads      head_id = -1, the 'argmin' loss: every head through one pass of both trunks, forward and backward
  two_pass       what needs none of the all-heads training kernels and is valid when all unselected loss weights are
                 zero: a no_grad all-heads inference forward with the same t_rand, the criteria read on the host, then a
                 head_id = best step
Prints one JSON line; reads nothing outside the repository (and --parent-lib).

The split of a step by kernel comes from two profiler runs of their own (kernel trace only, no counters), one way each:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR_A -- python profiles/tools/time_multihead_train.py --only single
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR_B -- python profiles/tools/time_multihead_train.py --only all_heads
    python profiles/tools/time_multihead_train.py --kernel-stats DIR_A DIR_B
--only WAY runs --warmup + --steps steps of that way and nothing else; --kernel-stats reads the two *kernel_stats.csv
files and prints, per group of kernels, ms and launches per step of both ways and the difference (no GPU needed)."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from humannerf_amd import _lib, scene
from humannerf_amd.config import cfg
from humannerf_amd.network import Network
from humannerf_amd.seeded import default_shapes, seeded_state
from humannerf_amd.train import Trainer

KEYS = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec', 'cnl_bbox_min_xyz',
        'cnl_bbox_scale_xyz', 'bgcolor']
START = 60000


def batch(dev):
    """The bench's training item: six 32 x 32 windows of the 512 x 512 synthetic frame, flat rays with targets."""
    fr = scene.synthetic_frame(H=512, W=512, focal_at_512=1700.0)
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in KEYS}
    idx = []
    for k in range(6):
        y0, x0 = 96 + 48 * k, 80 + 56 * k
        yy, xx = np.meshgrid(np.arange(y0, y0 + 32), np.arange(x0, x0 + 32), indexing='ij')
        idx.append((yy * 512 + xx).reshape(-1))
    idx = torch.from_numpy(np.concatenate(idx)).to(dev)
    tb = dict(data, rays=data['rays'][:, idx].contiguous(), near=data['near'][idx].contiguous(), far=data['far'][idx].contiguous())
    gen = torch.Generator(device=dev).manual_seed(1)
    tb['target_rgbs'] = torch.rand(6144, 3, device=dev, generator=gen)
    tb['t_rand'] = torch.rand(6144, 128, device=dev, generator=gen)
    return tb


def network(heads, dev):
    """A seeded network with ``heads`` heads (0: the single-head one) and its Trainer at the steady-state iteration."""
    state = seeded_state(default_shapes(), 0)
    keep = (cfg.get('multihead'), cfg.canonical_mlp.get('multihead'))
    if heads:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'tests'))
        from multihead_cases import multihead_state
        state = multihead_state(state, heads)
        cfg.canonical_mlp.multihead = {'enable': True, 'head_depth': 1}
        cfg.multihead = {'head_num': heads, 'split': 'argmin'}
    try:
        net = Network()
    finally:
        for node, key, val in ((cfg, 'multihead', keep[0]), (cfg.canonical_mlp, 'multihead', keep[1])):
            if not heads:
                continue
            if val is None:
                node.pop(key, None)
            else:
                node[key] = val
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    net = net.to(dev).train()
    tr = Trainer(net)
    tr.iter = START
    return net, tr


GROUPS = (('K4 composite_fwd', ('composite_kernel',)), ("K4' composite_bwd", ('composite_bwd',)),
          ('head dW / db', ('mlp_dwh_head', 'mlp_dw_head')),
          ('canonical forward-train', ('canonical_f16x3_kernel', 'canonical_f32_kernel')),
          ('canonical chain', ('canonical_bwd',)), ('canonical pack', ('pack_layer', 'pack_bwd', 'layer_amax')),
          ('hidden dW', ('mlp_dwh_', 'mlp_dw_', 'mlp_dw16')), ('non-rigid MLP', ('nonrigid_',)), ('K1, K1\'', ('sample_warp',)))


def kernel_stats(dir_a, dir_b, steps):
    """Per group of kernels: ms and launches per step of the two profiled ways, and b - a."""
    import csv
    import glob

    def load(d):
        files = sorted(glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True))
        assert files, 'no *kernel_stats.csv under %s' % d
        out = {}
        for r in csv.DictReader(open(files[-1])):
            name = r['Name']
            group = next((g for g, keys in GROUPS if any(k in name for k in keys)), 'everything else')
            ms, calls = out.get(group, (0.0, 0))
            out[group] = (ms + float(r['TotalDurationNs']) / 1e6 / steps, calls + int(r['Calls']))
        return out
    a, b = load(dir_a), load(dir_b)
    rows = {g: {'a_ms': round(a.get(g, (0, 0))[0], 4), 'b_ms': round(b.get(g, (0, 0))[0], 4),
                'a_launches': round(a.get(g, (0, 0))[1] / steps, 2), 'b_launches': round(b.get(g, (0, 0))[1] / steps, 2),
                'diff_ms': round(b.get(g, (0, 0))[0] - a.get(g, (0, 0))[0], 4)} for g in sorted(set(a) | set(b))}
    rows['total'] = {'a_ms': round(sum(v[0] for v in a.values()), 4), 'b_ms': round(sum(v[0] for v in b.values()), 4)}
    rows['total']['diff_ms'] = round(rows['total']['b_ms'] - rows['total']['a_ms'], 4)
    print(json.dumps({'steps_profiled': steps, 'kernel_ms_per_step': rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--heads', type=int, default=4)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--only', default=None, help='run this one way (for a profiler) and print nothing')
    ap.add_argument('--kernel-stats', nargs=2, default=None, metavar=('DIR_A', 'DIR_B'))
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(*args.kernel_stats, steps=args.steps + args.warmup)
    dev = torch.device('cuda:0')
    cfg.perturb, cfg.N_samples = 1.0, 128
    cfg.train.lossweights = {'lpips': 0.0, 'mse': 0.2, 'l1': 0.0}
    cfg.amd.train_heads = True
    tb = batch(dev)
    net1, tr1 = network(0, dev)
    netH, trH = network(args.heads, dev)
    own = _lib.load_open()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name, (res, argtypes) in _lib.SIGNATURES.items():
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = res, argtypes

    def two_pass():
        with torch.no_grad():
            out = netH(**tb, head_id=-1, iter_val=float(trH.iter))
        crit = torch.stack([((rgb - tb['target_rgbs']) ** 2).mean() for rgb in out['rgb']])
        best = int(crit.argmin().item())                            # the host read the one-pass loss makes too
        return trH.train_step(dict(tb, head_id=best))

    def with_parent():
        _lib._lib = parent
        try:
            return tr1.train_step(tb)
        finally:
            _lib._lib = own

    ways = {'single': lambda: tr1.train_step(tb), 'head': lambda: trH.train_step(dict(tb, head_id=1)),
            'all_heads': lambda: trH.train_step(dict(tb, head_id=-1)), 'two_pass': two_pass}
    if parent is not None:
        ways['parent_single'] = with_parent
    if args.only:
        for _ in range(args.warmup + args.steps):
            ways[args.only]()
        torch.cuda.synchronize()
        return
    times = {k: [] for k in ways}
    for rep in range(args.repeats):
        order = list(ways) if rep % 2 == 0 else list(ways)[::-1]
        for name in order:
            fn = ways[name]
            for _ in range(args.warmup):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(round(a.elapsed_time(b) / args.steps, 4))
    res = {'heads': args.heads, 'rays': 6144, 'samples': 128, 'steps': args.steps, 'ms_per_step': times,
           'best_head_last': trH.best_head}
    m = {k: min(v) for k, v in times.items()}
    res['all_heads_over_single'] = round(m['all_heads'] / m['single'], 4)
    res['all_heads_over_two_pass'] = round(m['all_heads'] / m['two_pass'], 4)
    res['head_over_single'] = round(m['head'] / m['single'], 4)
    if parent is not None:
        (lo, hi), (slo, shi) = (min(times['parent_single']), max(times['parent_single'])), (min(times['single']), max(times['single']))
        res['single_vs_parent'] = {'single': [slo, shi], 'parent': [lo, hi], 'single_inside_parent_spread': bool(lo <= slo and shi <= hi),
                                   'spreads_overlap': bool(slo <= hi and lo <= shi)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
