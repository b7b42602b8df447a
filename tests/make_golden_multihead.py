"""Generate tests/golden/multihead.npz: the reference's multi-head canonical MLP (canonical_mlp.multihead.enable,
head_depth 1) with H = 3 and H = 8 heads on seeded weights.

    python tests/make_golden_multihead.py <reference checkout>

Needs the reference checkout (it is imported read-only, on the CPU; only its numerical outputs are stored) and no GPU.
Per H the file holds
  * the reference's own CanonicalMLP class on the stored positional encodings ``pe`` (300 points): ``H<H>/cls_all`` the
    list its head_id = -1 returns, ``H<H>/cls_each`` its output for every head_id = h, both stacked (H, P, 4);
  * the reference Network.forward on the CPU with head_id = h for every h, on the first 200 rays of the default golden
    frame (tests/golden/meta.json 'frame') at S = 16, iter_val 1e7: ``H<H>/rgb`` (H, 200, 3), ``alpha``, ``depth``
    (H, 200).  (The reference's own head_id = -1 branch of Network.forward is not driven: it never fills 'offsets'.)
Weights: humannerf_amd.seeded.seeded_state(default shapes, seed 0) with the head tensors of
tests/multihead_cases.head_tensors -- nothing but their seed is stored."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
N_RAYS, N_POINTS = 200, 300


def main(ref):
    import torch
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    import json
    import multihead_cases as mc
    from oracle import make_golden, oracle
    make_golden.REF = ref
    cfg, create_network = make_golden.import_reference()
    from humannerf_amd import scene
    from humannerf_amd.seeded import default_shapes, seeded_state
    torch.set_num_threads(8)
    base = seeded_state(default_shapes(), seed=0)
    with open(os.path.join(HERE, 'golden', 'meta.json')) as f:
        frame_args = {k: v for k, v in json.load(f)['frame'].items() if k != 'seed'}
    fr = scene.synthetic_frame(**frame_args)
    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
            'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']
    tens = {k: torch.from_numpy(np.ascontiguousarray(fr[k])) for k in keys}
    tens['rays'] = tens['rays'][:, :N_RAYS].contiguous()
    tens['near'], tens['far'] = tens['near'][:N_RAYS].contiguous(), tens['far'][:N_RAYS].contiguous()
    xyz = np.random.RandomState(5).uniform(-1.3, 1.3, (N_POINTS, 3)).astype(np.float32)
    pe = oracle.fourier_pe(torch.from_numpy(xyz), 10)
    save = {'pe': pe.numpy(), 'head_seed': np.int64(mc.HEAD_SEED), 'n_rays': np.int64(N_RAYS), 'S': np.int64(mc.FIXTURE_S)}
    cfg.N_samples, cfg.perturb, cfg.ignore_non_rigid_motions = mc.FIXTURE_S, 0.0, False
    cfg.canonical_mlp.multihead.enable = True
    cfg.canonical_mlp.multihead.head_depth = 1
    for H in mc.FIXTURE_HEADS:
        cfg.multihead.head_num = H
        net = create_network()
        state = mc.multihead_state(base, H)
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: v.shape for k, v in state.items()}
        net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
        net.eval()
        cnl = net.cnl_mlp
        hid = lambda h: torch.full((N_POINTS, 1), h, dtype=torch.int64)
        with torch.no_grad():
            every = cnl(pos_embed=pe, head_id=hid(-1))
            assert isinstance(every, list) and len(every) == H
            save['H%d/cls_all' % H] = np.stack([o.numpy() for o in every])
            save['H%d/cls_each' % H] = np.stack([cnl(pos_embed=pe, head_id=hid(h)).numpy() for h in range(H)])
            outs = [net(**tens, head_id=torch.tensor(h), iter_val=1e7) for h in range(H)]
        for k in ('rgb', 'alpha', 'depth'):
            save['H%d/%s' % (H, k)] = np.stack([o[k].numpy() for o in outs])
        print('H', H, 'alpha mean per head', save['H%d/alpha' % H].mean(axis=1))
    path = os.path.join(HERE, 'golden', 'multihead.npz')
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
