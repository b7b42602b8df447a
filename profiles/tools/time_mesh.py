"""Milliseconds of the three passes of Network.extract_canonical_mesh from HIP events, at N = 256 and 512:
density lattice (hnrf_density_grid), extraction (hnrf_mesh_count + hnrf_mesh_emit, without the host read of the
counts between them) and vertex colours (hnrf_canonical_fwd at the vertices + sigmoid).  Seeded network with the
sigma bias raised by 5 (tests/test_gpu_mesh.py), level 10, the synthetic frame's canonical bbox.  One JSON line per N.

    python profiles/tools/time_mesh.py [--reps 5] [--mode f16x3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from humannerf_amd import ops, scene  # noqa: E402
from humannerf_amd.config import cfg  # noqa: E402
from humannerf_amd.network import Network  # noqa: E402
from humannerf_amd.seeded import default_shapes, seeded_state, with_density  # noqa: E402


def timed(fn, reps):
    """Median over ``reps`` of the event time of fn() (after one warm-up call); returns (ms, last result)."""
    out = fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--mode', default='f16x3', choices=['f32', 'f16x3'])
    ap.add_argument('--level', type=float, default=10.0)
    args = ap.parse_args()
    cfg.amd.mlp_mode = args.mode
    dev = torch.device('cuda:0')
    net = Network()
    state = with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    net = net.to(dev).eval()
    fr = scene.synthetic_frame(H=64, W=64)
    bmin = torch.from_numpy(fr['cnl_bbox_min_xyz']).to(dev)
    bmax = torch.from_numpy(fr['cnl_bbox_max_xyz']).to(dev)
    scale = torch.from_numpy(fr['cnl_bbox_scale_xyz']).to(dev)
    with torch.no_grad():
        vol = net._weight_volume(torch.from_numpy(fr['motion_weights_priors']).to(dev))
        packed = net._canonical_packed()
        for N in (256, 512):
            t_density, density = timed(lambda: ops.density_grid(packed, vol, bmin, bmax, scale, N, args.mode), args.reps)
            ws = ops.mesh_workspace(N, dev)
            V, F = ops.mesh_count(density, args.level, ws)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            lib = ops._lib.load()

            def count():
                ops._lib.check(lib.hnrf_mesh_count(density.data_ptr(), N, args.level, ws.data_ptr(), ws.numel() * 4,
                                                   counts.data_ptr(), ops._stream()), 'hnrf_mesh_count')
            t_count, _ = timed(count, args.reps)
            t_emit, (verts, faces) = timed(lambda: ops.mesh_emit(density, args.level, bmin, bmax, ws, V, F), args.reps)
            t_color, _ = timed(lambda: torch.sigmoid(ops.canonical(verts, packed, args.mode)[:, :3]), args.reps)
            print(json.dumps({'N': N, 'mode': args.mode, 'vertices': V, 'faces': F,
                              'density_ms': round(t_density, 3), 'extract_ms': round(t_count + t_emit, 3),
                              'count_ms': round(t_count, 3), 'emit_ms': round(t_emit, 3), 'colors_ms': round(t_color, 3),
                              'density_points_per_s': round(N ** 3 / t_density * 1e3)}), flush=True)
            del density, ws, verts, faces
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
