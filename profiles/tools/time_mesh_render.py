"""Frame time of the mesh preview (Network.pose_vertices + raster.rasterize) against the volume renderer
(Network.forward) on the same frame, from HIP events with the profiler off.  Seeded network with the sigma bias raised
by 5 (tests/test_gpu_mesh.py), level 10, the synthetic frame (pose seed 3) whose every pixel ray hits the canonical
bbox.  For mesh resolutions N x image sizes x cull none / back, one JSON line each: median and spread over --frames
frames (after --warmup frames of that shape) of forward skinning alone, of the rasteriser alone (clear + setup +
visibility + resolve) and of the two together, frames/s of the loop by the wall clock (launches queued back to back,
one synchronisation at the end), the volume render's time and the ratio, and the agreement of the two pictures
(silhouette IoU at alpha > 0.5, median |depth difference| where both cover, against the volume's depth as it is
and divided by its alpha).  The per-kernel split comes from a run of
its own under ``rocprofv3 --kernel-trace --stats`` (``--no-volume --configs N,size,cull``).

With a diagnostic build of hnrf_raster.hip (-DHNRF_RASTER_COUNT [-DHNRF_RASTER_EARLY_OUT], selected through
HNRF_LIB_PATH) ``--counts`` also reports the samples owned and the atomics issued per frame (the counting itself costs
several times the kernel: times come from builds without it).

    python profiles/tools/time_mesh_render.py [--frames 200] [--warmup 10] [--configs 256,512,back ...] [--no-volume] [--counts]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from humannerf_amd import ops, raster, scene  # noqa: E402
from humannerf_amd.config import cfg  # noqa: E402
from humannerf_amd.network import Network  # noqa: E402
from humannerf_amd.seeded import default_shapes, seeded_state, with_density  # noqa: E402


def event_ms(fn, frames, warmup):
    """Event time of each of ``frames`` calls of fn() after ``warmup`` calls -> sorted list of ms, last result."""
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
    q = lambda p: round(ms[min(len(ms) - 1, int(p * len(ms)))], 4)
    return {'median': q(0.5), 'min': round(ms[0], 4), 'p10': q(0.1), 'p90': q(0.9), 'max': round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--level', type=float, default=10.0)
    ap.add_argument('--configs', nargs='*', default=None, help='N,size,cull triples; default: {256,512} x {512,1024} x {none,back}')
    ap.add_argument('--no-volume', action='store_true')
    ap.add_argument('--counts', action='store_true')
    args = ap.parse_args()
    configs = [tuple(c.split(',')) for c in args.configs] if args.configs else \
        [(N, s, c) for N in ('256', '512') for s in ('512', '1024') for c in ('none', 'back')]
    dev = torch.device('cuda:0')
    net = Network()
    state = with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    net = net.to(dev).eval()
    cfg.perturb, cfg.N_samples, cfg.amd.diagnostics = 0., 128, False      # the render loops' lean forward
    meshes, volume = {}, {}
    for N, size, cull in configs:
        N, size = int(N), int(size)
        cam = scene.synthetic_frame(H=size, W=size, pose_seed=3, pose_scale=0.3, camera_only=True)
        priors = torch.from_numpy(cam['motion_weights_priors']).to(dev)
        cam['motion_weights_priors'] = priors                     # resident: the weight volume is kept by identity
        with torch.no_grad():
            if N not in meshes:
                meshes.clear()
                torch.cuda.empty_cache()
                meshes[N] = net.extract_canonical_mesh(cam['cnl_bbox_min_xyz'], cam['cnl_bbox_max_xyz'], priors,
                                                       resolution=N, level=args.level)
            verts, faces, colors = meshes[N]
            motion_Rs, motion_Ts, vol = net.frame_motion(cam)
            bmin = torch.from_numpy(cam['cnl_bbox_min_xyz']).to(dev)
            scale = torch.from_numpy(cam['cnl_bbox_scale_xyz']).to(dev)
            posed = ops.forward_skin(verts, motion_Rs, motion_Ts, vol, bmin, scale)
            kw = dict(cull=cull, shade='color')
            bg = cam['bgcolor'] / 255.
            t_skin, _ = event_ms(lambda: ops.forward_skin(verts, motion_Rs, motion_Ts, vol, bmin, scale), args.frames, args.warmup)
            t_rast, _ = event_ms(lambda: raster.rasterize(posed, faces, colors, cam['K'], cam['E'], size, size, bgcolor=bg, **kw),
                                 args.frames, args.warmup)
            t_both, out = event_ms(lambda: net.render_mesh(verts, faces, colors, cam, **kw), args.frames, args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.frames):
                out = net.render_mesh(verts, faces, colors, cam, **kw)
            torch.cuda.synchronize()
            fps = args.frames / (time.perf_counter() - t0)
            row = {'N': N, 'image': size, 'cull': cull, 'vertices': verts.shape[0], 'faces': faces.shape[0],
                   'covered_pixels': int((out['tri_id'] >= 0).sum()), 'skin_ms': spread(t_skin), 'raster_ms': spread(t_rast),
                   'pose_and_raster_ms': spread(t_both), 'loop_frames_per_s': round(fps, 1)}
            if args.counts:
                ws = ops.raster_workspace(verts.shape[0], faces.shape[0], size, size, dev)
                need = ops._lib.load().hnrf_raster_workspace_bytes(verts.shape[0], faces.shape[0], size, size)
                head = ws.view(torch.int32)[need // 4 - 64:need // 4 - 58].cpu().numpy()      # the header: last 256 bytes
                u64 = head[2:6].astype(np.uint32).view(np.uint64)
                row.update(large_triangles=int(head[0]), owned_samples=int(u64[0]), atomics_issued=int(u64[1]))
            if not args.no_volume:
                if size not in volume:
                    fr = scene.synthetic_frame(H=size, W=size, pose_seed=3, pose_scale=0.3)
                    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'dst_posevec', 'cnl_bbox_min_xyz',
                            'cnl_bbox_scale_xyz', 'bgcolor']
                    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in keys}
                    data['motion_weights_priors'] = priors
                    t_vol, res = event_ms(lambda: net(**data, iter_val=1e7), 5, 2)
                    mask = torch.from_numpy(fr['ray_mask'].reshape(-1)).to(dev)
                    full = lambda t: torch.zeros(size * size, device=dev).masked_scatter_(mask, t.reshape(-1)).reshape(size, size)
                    volume[size] = (t_vol, full(res['alpha']), full(res['depth']), int(mask.sum()))
                t_vol, v_alpha, v_depth, rays = volume[size]
                a_m, a_v = out['alpha'] > 0.5, v_alpha > 0.5
                both = a_m & a_v
                row.update(volume_ms=spread(t_vol), volume_rays=rays,
                           volume_over_mesh=round(spread(t_vol)['median'] / spread(t_both)['median'], 1),
                           silhouette_iou=round(float(both.sum()) / max(1.0, float((a_m | a_v).sum())), 4),
                           median_abs_depth_diff=round(float((out['depth'] - v_depth)[both].abs().median()), 5),
                           # (the volume depth is sum w z with sum w = alpha < 1 on a translucent field: also per unit alpha)
                           median_abs_depth_diff_per_alpha=round(float((out['depth'] - v_depth / v_alpha.clamp(min=1e-6))[both].abs().median()), 5),
                           volume_alpha_median=round(float(v_alpha[both].median()), 3))
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
