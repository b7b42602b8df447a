"""The numbers of profiles/gltf_export.txt, from one process on one MI355X: the seeded network (sigma bias raised by 5,
level 10, as profiles/tools/time_mesh.py), its canonical mesh at N = 256, and 16 frames of scene.synthetic_frame poses
(pose_seed 0..15, pose_scale 0.3).

  hnrf_skin_weights, K = 4 and 8: ms per call from HIP events around ``--calls`` back-to-back calls, median of
      ``--reps`` windows, and ms per million vertices;
  hnrf_skin_lbs against hnrf_forward_skin per frame, the windows alternating;
  per K: the size of the .glb with the 16 frames, kept (min / mean) and the skinning error |skin_lbs - pose_vertices|
      in metres (max / mean over vertices and frames), the pose refiner acting.

One JSON line each.  The seeded network is a noise field: the error figures say nothing about a trained avatar.

    python profiles/tools/time_gltf.py [--resolution 256] [--reps 7] [--calls 20] [--out DIR]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

from humannerf_amd import gltf, ops, scene, skin  # noqa: E402
from humannerf_amd.network import Network  # noqa: E402
from humannerf_amd.seeded import default_shapes, seeded_state, with_density  # noqa: E402


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=256)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--level', type=float, default=10.0)
    ap.add_argument('--out', default='.')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_gltf.py measures on the GPU'
    dev = torch.device('cuda:0')
    net = Network()
    state = with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    net = net.to(dev).eval()
    frames = [scene.synthetic_frame(H=64, W=64, pose_seed=s, pose_scale=0.3) for s in range(args.frames)]
    fr = frames[0]
    priors = torch.from_numpy(fr['motion_weights_priors']).to(dev)
    frames = [dict(f, motion_weights_priors=priors) for f in frames]
    verts, faces, colors = net.extract_canonical_mesh(fr['cnl_bbox_min_xyz'], fr['cnl_bbox_max_xyz'], priors,
                                                      resolution=args.resolution, level=args.level)
    V = verts.shape[0]
    print(json.dumps({'resolution': args.resolution, 'vertices': V, 'faces': int(faces.shape[0])}), flush=True)
    bmin = torch.from_numpy(fr['cnl_bbox_min_xyz']).to(dev)
    scale = torch.from_numpy(fr['cnl_bbox_scale_xyz']).to(dev)
    with torch.no_grad():
        vol = net._weight_volume(priors)
        Rs, Ts, _ = net.frame_motion(frames[1])
        mats = skin.joint_matrices(Rs, Ts)
        for K in (4, 8):
            call = lambda: skin.skin_weights(verts, vol, bmin, scale, k=K)
            window(call, 3)
            ms = median([window(call, args.calls) for _ in range(args.reps)])
            print(json.dumps({'kernel': 'hnrf_skin_weights', 'K': K, 'ms': round(ms, 4),
                              'ms_per_million_vertices': round(ms / V * 1e6, 4)}), flush=True)
        fwd = lambda: ops.forward_skin(verts, Rs, Ts, vol, bmin, scale)
        for K in (4, 8):
            joints, weights, _ = skin.skin_weights(verts, vol, bmin, scale, k=K)
            lbs = lambda: skin.skin_lbs(verts, joints, weights, mats)
            window(lbs, 3), window(fwd, 3)
            t_lbs, t_fwd = [], []
            for _ in range(args.reps):
                t_lbs.append(window(lbs, args.calls))
                t_fwd.append(window(fwd, args.calls))
            print(json.dumps({'per_frame': 'hnrf_skin_lbs vs hnrf_forward_skin', 'K': K, 'skin_lbs_ms': round(median(t_lbs), 4),
                              'forward_skin_ms': round(median(t_fwd), 4),
                              'skin_lbs_ms_range': [round(min(t_lbs), 4), round(max(t_lbs), 4)],
                              'forward_skin_ms_range': [round(min(t_fwd), 4), round(max(t_fwd), 4)]}), flush=True)
        for K in (4, 8):
            joints, weights, kept = net.skin_weights(verts, frames[0], k=K)
            worst, mean, rots = 0.0, [], []
            for f in frames:
                mRs, mTs, _ = net.frame_motion(f)
                d = skin.skin_lbs(verts, joints, weights, skin.joint_matrices(mRs, mTs)) - net.pose_vertices(verts, f)
                d = torch.sqrt((d * d).sum(1))
                worst, mean = max(worst, float(d.max())), mean + [float(d.mean())]
                rvec = net.refiner_rvec(f)
                rots.append(gltf.refined_rotations(f['dst_Rs'], None if rvec is None else rvec.cpu().numpy()))
            path = os.path.join(args.out, 'avatar_K%d.glb' % K)
            size = gltf.write_glb(path, verts, faces, colors, joints, weights, fr['cnl_gtfms'], dst_Rs=np.stack(rots),
                                  dst_Ts=np.stack([f['dst_Ts'] for f in frames]))
            os.remove(path)
            print(json.dumps({'export': 'K = %d, %d frames' % (K, len(frames)), 'file_bytes': size,
                              'kept_min': round(float(kept.min()), 4), 'kept_mean': round(float(kept.mean()), 4),
                              'skin_error_max_m': float('%.3e' % worst), 'skin_error_mean_m': float('%.3e' % np.mean(mean))}),
                  flush=True)


if __name__ == '__main__':
    main()
