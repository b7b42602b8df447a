"""What the shared evaluation of underflowing inputs buys the all-heads frame, from HIP events with the profiler off.
One JSON line per process: the bench frame (512 x 512 rays x 128 samples, bench.py's camera), H = --heads, 11-output and
lean form, these legs taken in turns (a, b, c, d, a, b, ...):

  all_on / all_off   forward(head_id=-1) with cfg.amd.share_underflow on / off
  one_on / one_off   forward(head_id=0), the single-head frame, with the option on / off

    python profiles/tools/time_multihead_shared.py [--heads 4] [--iters 20] [--warmup 3] [--legs all_on,all_off,...]

The library is the one humannerf_amd._lib loads: HNRF_LIB_PATH names another build, e.g. the parent commit's.  A library
without the entries of include/hnrf_heads_shared.h runs the legs it has -- all_off and one_on, the two this change must
not move -- and says so ("shared_heads_entries": false).  The caller runs this build and the parent's in turns, one
process each, each at least twice, in one job, every process under its own timeout.

Reported against (profiles/multihead_shared.txt): (a) all_on / all_off <= one_on / one_off + 0.05 of the same process;
(b) one_on of this build against the parent's inside the spread of its own repeats.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from humannerf_amd import _lib, scene  # noqa: E402
from humannerf_amd.config import cfg  # noqa: E402
from humannerf_amd.seeded import default_shapes, seeded_state  # noqa: E402
from time_multihead import head_state, interleaved_ms  # noqa: E402  (profiles/tools, next to this file)

LEGS = {'all_on': (-1, True), 'all_off': (-1, False), 'one_on': (0, True), 'one_off': (0, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--heads', type=int, default=4)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--legs', default=None, help='comma-separated, of ' + ', '.join(LEGS))
    args = ap.parse_args()
    from humannerf_amd.network import Network
    dev = torch.device('cuda:0')
    has = hasattr(_lib.load(), 'hnrf_render_frame_heads_shared_fwd')
    legs = args.legs.split(',') if args.legs else (list(LEGS) if has else ['all_off', 'one_on'])
    if not has and 'all_on' in legs:
        raise SystemExit('%s has no hnrf_render_frame_heads_shared_fwd: all_on cannot run' % _lib.LIB_PATH)
    H = args.heads
    cfg.canonical_mlp.multihead = {'enable': True, 'head_depth': 1}
    cfg.multihead = {'head_num': H}
    net = Network()
    state = seeded_state(default_shapes(), seed=0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in head_state(state, H).items()}, strict=True)
    net = net.to(dev).eval()
    cfg.perturb, cfg.N_samples, cfg.ignore_non_rigid_motions = 0., 128, False
    fr = scene.synthetic_frame(H=512, W=512, focal_at_512=1700.0, pose_seed=0)
    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
            'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in keys}
    res = {'lib': os.path.relpath(_lib.LIB_PATH), 'shared_heads_entries': has, 'heads': H,
           'rays': int(data['rays'].shape[1]), 'samples': 128, 'chunk': int(cfg.chunk),
           'overlap_warp': bool(cfg.amd.overlap_warp)}

    def leg(name):
        head, share = LEGS[name]

        def run():
            cfg.amd.share_underflow = share
            return net(**data, head_id=head, iter_val=1e7)
        return run

    with torch.no_grad():
        for diag in (True, False):
            cfg.amd.diagnostics = diag
            t = interleaved_ms({k: leg(k) for k in legs}, args.iters, args.warmup)
            share = {}
            for k in legs:                                      # the share of shared samples of each shared leg
                if LEGS[k][1]:
                    leg(k)()
                    share[k] = round(net.shared_sample_share(), 6)
            t['shared_share'] = share
            for a, b in (('all_on', 'all_off'), ('one_on', 'one_off')):
                if a in t and b in t:
                    t[a + '_over_' + b] = round(t[a]['median'] / t[b]['median'], 4)
            if 'all_on' in t and 'one_on' in t:
                t['all_on_over_one_on'] = round(t['all_on']['median'] / t['one_on']['median'], 4)
            res['11-output' if diag else 'lean'] = t
        net.check_f16_range(wait=True)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
