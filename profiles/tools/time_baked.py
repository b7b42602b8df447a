"""Baked canonical grid (cfg.amd.canonical = 'baked') against the exact renderer on the bench frame (512 x 512 rays x
128 samples, seeded network, bench.py's frame), from HIP events with the profiler off.  One JSON line per step:

  bake      per N: time of Network.bake_canonical's device work (ops.bake_canonical), saturated values;
  chunk     per N: the sampler's time per ray chunk of 32 768 x 128 from the event pairs the frame pipeline records
            around it, with its bytes/s (28 B streamed + 64 B gathered per sample), beside the canonical f16x3 kernel's
            time from the same event pairs of the exact frame of the same run, and the ratio;
  frame     per N x {11-output, lean, lean + cull_eps 1e-9} x {non-rigid MLP on, off}: frame time exact and baked;
  fidelity  per N: PSNR and max |d rgb| of the baked frame against the exact one;
  nonrigid  the per-frame offset grid (cfg.amd.nonrigid = 'baked') at canonical N = --nr-canonical (256), per M of
            --nr-sizes: (a) today's baked frame (non-rigid MLP), lean and 11-output; K2's time per ray chunk from event
            pairs around ops.nonrigid on every chunk's own x_skel (lean form: no offsets output) and its sum over the
            frame's chunks; the canonical-only sampler per chunk from the pipeline's event pairs; (b) both baked: the
            per-frame bake (ops.bake_nonrigid, resident workspace), the fused sampler per chunk from the pipeline's
            event pairs, the frame lean and 11-output with the grid held and with a fresh dst_posevec tensor per frame
            (one bake per frame, the render loops' case); and the acceptance figure: non-rigid work of (b) = bake +
            n_chunks x (fused - canonical-only sampler) over K2's time in (a);
  nonrigid_fidelity  per M: PSNR, max / mean |d rgb| and |d alpha| of (b) against (a) and against the exact frame.

    python profiles/tools/time_baked.py [--sizes 128 256 512] [--frames 5] [--warmup 2] [--density]
                                        [--nr-sizes 64 128 256] [--nr-canonical 256]

--density raises the sigma bias by 5 (the mesh tests' network) so that the picture is not nearly empty.  Every step
stands alone: the caller runs one step per process under its own timeout (--step bake|chunk|frame|fidelity|nonrigid|
nonrigid_fidelity), chained so that a failure ends the run; without --step the first four run in this process.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from humannerf_amd import ops, scene  # noqa: E402
from humannerf_amd.config import cfg  # noqa: E402
from humannerf_amd.network import Network  # noqa: E402
from humannerf_amd.seeded import default_shapes, seeded_state, with_density  # noqa: E402


def event_ms(fn, frames, warmup):
    for _ in range(warmup):
        out = fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(frames)]
    for a, b in ev:
        a.record()
        out = fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev), out


def spread(ms):
    return {'median': round(ms[len(ms) // 2], 4), 'min': round(ms[0], 4), 'max': round(ms[-1], 4), 'n': len(ms)}


def chunk_ms(net, data, frames, warmup):
    """Per-chunk times of whatever stands in K3's place, from the pipeline's own event pairs (full chunks only)."""
    for _ in range(warmup):
        net(**data, iter_val=1e7)
    net.mlp_event_log = []
    for _ in range(frames):
        net(**data, iter_val=1e7)
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in net.mlp_event_log]
    net.mlp_event_log = None
    return sorted(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[128, 256, 512])
    ap.add_argument('--frames', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--density', action='store_true')
    ap.add_argument('--nr-sizes', type=int, nargs='*', default=[64, 128, 256])
    ap.add_argument('--nr-canonical', type=int, default=256)
    ap.add_argument('--step', choices=['bake', 'chunk', 'frame', 'fidelity', 'nonrigid', 'nonrigid_fidelity'], default=None)
    args = ap.parse_args()
    steps = [args.step] if args.step else ['bake', 'chunk', 'frame', 'fidelity']
    dev = torch.device('cuda:0')
    state = seeded_state(default_shapes(), seed=0)
    if args.density:
        state = with_density(state, bias_delta=5.0)
    net = Network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    net = net.to(dev).eval()
    fr = scene.synthetic_frame(H=512, W=512, focal_at_512=1700.0, pose_seed=0)
    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
            'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'cnl_bbox_max_xyz', 'bgcolor']
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in keys}
    R, S = data['rays'].shape[1], 128
    cfg.perturb, cfg.N_samples, cfg.amd.mlp_mode = 0., S, 'f16x3'
    P = int(cfg.chunk) * S
    tag = {'network': 'seeded' + ('+density5' if args.density else ''), 'rays': R, 'samples': S}

    def set_form(form, nonrigid):
        cfg.amd.diagnostics = form == 'full'
        cfg.amd.cull_eps = 1e-9 if form == 'lean_culled' else 0.0
        cfg.ignore_non_rigid_motions = not nonrigid

    with torch.no_grad():
        if 'bake' in steps:
            bmin, bmax = data['cnl_bbox_min_xyz'], data['cnl_bbox_max_xyz']
            packed = net._canonical_packed()
            for N in args.sizes:
                ms, (grid, sat) = event_ms(lambda: ops.bake_canonical(packed, bmin, bmax, N, 'f16x3', want_saturated=True),
                                           3, 1)
                print(json.dumps(dict(tag, step='bake', N=N, grid_MB=round(grid.numel() * 2 / 1e6, 1), bake_ms=spread(ms),
                                      saturated=int(sat), max_abs=float(grid.float().abs().max()))), flush=True)
                del grid
        if 'chunk' in steps:
            set_form('lean', True)
            cfg.amd.canonical = 'mlp'
            mlp = chunk_ms(net, data, args.frames, args.warmup)
            cfg.amd.canonical = 'baked'
            for N in args.sizes:
                cfg.amd.bake_resolution = N
                smp = chunk_ms(net, data, args.frames, args.warmup)
                med = smp[len(smp) // 2]
                print(json.dumps(dict(tag, step='chunk', N=N, chunk_samples=P, sampler_ms=spread(smp),
                                      canonical_f16x3_ms=spread(mlp),
                                      sampler_over_canonical=round(med / mlp[len(mlp) // 2], 4),
                                      sampler_TB_per_s=round(P * 92 / (med * 1e-3) / 1e12, 3))), flush=True)
            net.set_baked_grid(None, None, None)
        if 'frame' in steps:
            for nonrigid in (True, False):
                for form in ('full', 'lean', 'lean_culled'):
                    set_form(form, nonrigid)
                    cfg.amd.canonical = 'mlp'
                    exact, _ = event_ms(lambda: net(**data, iter_val=1e7), args.frames, args.warmup)
                    row = dict(tag, step='frame', form=form, nonrigid=nonrigid, exact_ms=spread(exact))
                    cfg.amd.canonical = 'baked'
                    for N in args.sizes:
                        cfg.amd.bake_resolution = N
                        net(**data, iter_val=1e7)                                   # (bakes)
                        b, _ = event_ms(lambda: net(**data, iter_val=1e7), args.frames, args.warmup)
                        row['baked_%d_ms' % N] = spread(b)
                        row['exact_over_baked_%d' % N] = round(exact[len(exact) // 2] / b[len(b) // 2], 2)
                    print(json.dumps(row), flush=True)
            net.set_baked_grid(None, None, None)
        if 'fidelity' in steps:
            set_form('lean', True)
            cfg.amd.canonical = 'mlp'
            exact = net(**data, iter_val=1e7)
            cfg.amd.canonical = 'baked'
            for N in args.sizes:
                cfg.amd.bake_resolution = N
                out = net(**data, iter_val=1e7)
                d = (out['rgb'] - exact['rgb']).double()
                mse = float((d * d).mean())
                print(json.dumps(dict(tag, step='fidelity', N=N, psnr_db=round(-10 * np.log10(mse), 2) if mse > 0 else None,
                                      max_abs_drgb=float(d.abs().max()), mean_abs_drgb=float(d.abs().mean()),
                                      max_abs_dalpha=float((out['alpha'] - exact['alpha']).abs().max()),
                                      exact_alpha_mean=float(exact['alpha'].mean()))), flush=True)
        if 'nonrigid' in steps:
            med = lambda ms: ms[len(ms) // 2]
            cfg.amd.canonical, cfg.amd.bake_resolution, cfg.amd.nonrigid = 'baked', args.nr_canonical, 'mlp'
            row = dict(tag, step='nonrigid', which='a: baked canonical, non-rigid MLP', N=args.nr_canonical)
            for form in ('lean', 'full'):
                set_form(form, True)
                net(**data, iter_val=1e7)                                           # (bakes the canonical grid)
                ms, _ = event_ms(lambda: net(**data, iter_val=1e7), args.frames, args.warmup)
                row['frame_%s_ms' % form] = spread(ms)
            set_form('lean', True)
            cnl_only = chunk_ms(net, data, args.frames, args.warmup)
            row['canonical_sampler_chunk_ms'] = spread(cnl_only)
            # K2 on every chunk's own samples, as the lean frame launches it
            Rs, Ts, vol = net.frame_motion(fr)
            nrc = cfg.non_rigid_motion_mlp
            from humannerf_amd.network import hann_window_weights
            hann = hann_window_weights(1e7, nrc.multires, nrc.kick_in_iter, nrc.full_band_iter).to(dev)
            packed = net._nonrigid_packed(data['dst_posevec']).clone()
            chunk, k2 = int(cfg.chunk), []
            for r0 in range(0, R, chunk):
                sl = slice(r0, min(r0 + chunk, R))
                _, x_skel, _, _ = ops.sample_warp(data['rays'][0][sl].contiguous(), data['rays'][1][sl].contiguous(),
                                                  data['near'].reshape(-1)[sl].contiguous(),
                                                  data['far'].reshape(-1)[sl].contiguous(), None, Rs, Ts, vol,
                                                  data['cnl_bbox_min_xyz'], data['cnl_bbox_scale_xyz'], S)
                xyz = torch.empty_like(x_skel)
                ms, _ = event_ms(lambda: ops.nonrigid(x_skel, hann, packed, 'f16x3', xyz_out=xyz), args.frames, args.warmup)
                k2.append(med(ms))
                del x_skel, xyz
            k2_total = sum(k2)
            row.update(k2_chunk_ms=[round(v, 4) for v in k2], k2_frame_ms=round(k2_total, 4), n_chunks=len(k2))
            print(json.dumps(row), flush=True)
            cfg.amd.nonrigid = 'baked'
            bmin, bmax = data['cnl_bbox_min_xyz'], data['cnl_bbox_max_xyz']
            for M in args.nr_sizes:
                cfg.amd.nonrigid_bake_resolution = M
                ws = ops.bake_nonrigid_workspace(M, dev)
                bake, _ = event_ms(lambda: ops.bake_nonrigid(packed, hann, bmin, bmax, M, 'f16x3', workspace=ws),
                                   args.frames, args.warmup)
                del ws
                row = dict(tag, step='nonrigid', which='b: both baked', N=args.nr_canonical, M=M,
                           grid_MB=round(M ** 3 * 8 / 1e6, 1), bake_ms=spread(bake))
                for form in ('lean', 'full'):
                    set_form(form, True)
                    net(**data, iter_val=1e7)
                    c0 = net.nonrigid_bake_count
                    ms, _ = event_ms(lambda: net(**data, iter_val=1e7), args.frames, args.warmup)
                    assert net.nonrigid_bake_count == c0                            # the grid is held
                    row['frame_%s_ms' % form] = spread(ms)
                    ms, _ = event_ms(lambda: net(**dict(data, dst_posevec=data['dst_posevec'].clone()), iter_val=1e7),
                                     args.frames, args.warmup)
                    assert net.nonrigid_bake_count == c0 + args.frames + args.warmup  # one bake per frame
                    row['frame_%s_bake_per_frame_ms' % form] = spread(ms)
                set_form('lean', True)
                fused = chunk_ms(net, data, args.frames, args.warmup)
                work = med(bake) + len(k2) * (med(fused) - med(cnl_only))
                row.update(fused_sampler_chunk_ms=spread(fused), nonrigid_work_ms=round(work, 4),
                           k2_frame_ms=round(k2_total, 4), work_over_k2=round(work / k2_total, 4),
                           fused_TB_per_s=round(P * (12 + 16 + 128) / (med(fused) * 1e-3) / 1e12, 3))
                if M == 128:
                    row['acceptance_at_most_0.2'] = bool(work / k2_total <= 0.2)
                print(json.dumps(row), flush=True)
            net.set_baked_grid(None, None, None)
            cfg.amd.nonrigid = 'mlp'
        if 'nonrigid_fidelity' in steps:
            set_form('lean', True)
            cfg.amd.canonical, cfg.amd.nonrigid = 'mlp', 'mlp'
            exact = net(**data, iter_val=1e7)
            cfg.amd.canonical, cfg.amd.bake_resolution = 'baked', args.nr_canonical
            today = net(**data, iter_val=1e7)
            cfg.amd.nonrigid = 'baked'

            def against(out, ref):
                d = (out['rgb'] - ref['rgb']).double()
                a = (out['alpha'] - ref['alpha']).double().abs()
                mse = float((d * d).mean())
                return {'psnr_db': round(-10 * np.log10(mse), 2) if mse > 0 else None, 'max_abs_drgb': float(d.abs().max()),
                        'mean_abs_drgb': float(d.abs().mean()), 'max_abs_dalpha': float(a.max()),
                        'mean_abs_dalpha': float(a.mean())}
            print(json.dumps(dict(tag, step='nonrigid_fidelity', which='a against exact', N=args.nr_canonical,
                                  **against(today, exact), exact_alpha_mean=float(exact['alpha'].mean()))), flush=True)
            for M in args.nr_sizes:
                cfg.amd.nonrigid_bake_resolution = M
                out = net(**data, iter_val=1e7)
                print(json.dumps(dict(tag, step='nonrigid_fidelity', N=args.nr_canonical, M=M,
                                      against_a=against(out, today), against_exact=against(out, exact))), flush=True)
            net.set_baked_grid(None, None, None)
            cfg.amd.nonrigid = 'mlp'
        net.check_f16_range(wait=True)


if __name__ == '__main__':
    main()
