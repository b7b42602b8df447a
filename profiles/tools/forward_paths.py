"""A sha256 per output tensor for every inference path of Network.forward, on one small frame: run it on two
checkouts (a process each) and diff the two outputs to see that a host-side change left every path's bits alone.
40 x 40 synthetic frame, seeded weights, 16 samples, three ray chunks with a ragged last one."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from humannerf_amd import scene
from humannerf_amd.config import cfg
from humannerf_amd.network import Network
from humannerf_amd.seeded import default_shapes, seeded_state

dev = torch.device('cuda:0')
net = Network(); net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state(default_shapes(), 0).items()}); net = net.to(dev).eval()
fr = scene.synthetic_frame(H=40, W=40, focal_at_512=1250.0)
KEYS = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec', 'cnl_bbox_min_xyz',
        'cnl_bbox_max_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']
data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])).to(dev) for k in KEYS}
N = data['rays'].shape[1]
cfg.perturb, cfg.N_samples, cfg.chunk = 0., 16, N // 3 + 1
cfg.pose_decoder.kick_in_iter = 5000                     # (the non-rigid MLP's is 10000: 100 / 7000 / 20000 straddle both)
assert -(-N // cfg.chunk) == 3 and N % cfg.chunk
DEFAULTS = dict(diagnostics=True, cull_eps=0.0, term_eps=0.0, canonical='mlp', nonrigid='mlp', bake_resolution=256,
                nonrigid_bake_resolution=128, share_underflow=True, overlap_warp=False, f16_range_guard='audit',
                mlp_mode='f16x3')
baked = dict(canonical='baked', bake_resolution=24)
baked_nr = dict(baked, nonrigid='baked', nonrigid_bake_resolution=24)
PATHS = [('diagnostic', {}, 1), ('lean', dict(diagnostics=False), 1),
         ('lean cull_eps 1e-9', dict(diagnostics=False, cull_eps=1e-9), 1),
         ('lean term_eps 1e-4', dict(diagnostics=False, term_eps=1e-4), 1),
         ('baked 24', baked, 1), ('baked 24 lean', dict(baked, diagnostics=False), 1),
         ('baked + nonrigid baked 24', baked_nr, 2), ('baked + nonrigid baked 24 lean', dict(baked_nr, diagnostics=False), 2),
         ('share_underflow off', dict(share_underflow=False), 1), ('share_underflow off lean', dict(diagnostics=False, share_underflow=False), 1),
         ('overlap_warp', dict(overlap_warp=True), 1), ('overlap_warp lean', dict(diagnostics=False, overlap_warp=True), 1),
         ('guard full', dict(f16_range_guard='full'), 1), ('guard audit', dict(f16_range_guard='audit'), 3),
         ('guard audit term_eps 1e-4', dict(diagnostics=False, term_eps=1e-4, f16_range_guard='audit'), 3),
         ('guard off', dict(f16_range_guard='off'), 1), ('mlp_mode f32', dict(mlp_mode='f32'), 1)]
print('rays %d chunk %d' % (N, cfg.chunk))
for iter_val in (100.0, 7000.0, 20000.0, 1e7):
    for name, opts, frames in PATHS:
        for k, v in dict(DEFAULTS, **opts).items():
            setattr(cfg.amd, k, v)
        net.weights_changed()                            # (a fresh pack, audit schedule and grids for every path)
        net.set_baked_grid(None, None, None)
        for f in range(frames):
            with torch.no_grad():
                out = net(**data, iter_val=iter_val)
            assert net.check_f16_range(wait=True) is False
            for k in sorted(out):
                print('iter %-9g %-32s frame %d %-24s %s' % (iter_val, name, f, k, hashlib.sha256(out[k].cpu().numpy().tobytes()).hexdigest()[:32]))
        print('iter %-9g %-32s shared share %.6f bakes %d %d watched %d' % (iter_val, name, net.shared_sample_share(), net.bake_count,
                                                                      net.nonrigid_bake_count, net.f16_range_watched))
