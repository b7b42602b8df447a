"""Generate tests/golden/viewdir.npz: the reference's view-dependent colour (canonical_mlp.view_dir, view_embed 'mlp',
multires_dir 4) on seeded weights.

    python tests/make_golden_viewdir.py <reference checkout>

Needs the reference checkout (it is imported read-only, on the CPU; only its numerical outputs are stored) and no GPU.
The file holds
  * ``pe`` (300, 63) and ``dirs`` (300, 3): positional encodings and (unnormalised) directions, and ``cls_raw`` (300, 4):
    the reference's own CanonicalMLP(view_dir=True) on them (dir_embed from the reference's embedder of normalize(dirs));
  * the reference Network.forward on the CPU on the first 200 rays of the default golden frame (tests/golden/meta.json
    'frame') at S = 16, iter_val 1e7, for view_dir_camera_only False and True: ``rgb`` (2, 200, 3), ``alpha``, ``depth``
    (2, 200).  The third row of ``rays`` is row 1 turned by tests/viewdir_cases.camera_rotation(), so the two differ;
  * the reference's loss.backward() on the grad_s64 case (tests/golden/meta.json: ray_stride 73, S = 64, iter_val 30000,
    training mode, view_dir_camera_only False) for the loss of tests/make_golden_multihead_train.py with the loss weights
    of its head 0: per parameter ``norm/<name>``, then ``grad/<name>`` in full up to 32 768 elements or ``head/<name>``
    (the first 4096), ``loss``, and ``noise_floor`` / ``noise_floor_cos``: the largest relative norm distance and the
    smallest cosine between these fp32 gradients and the fp64 twin (tests/viewdir_cases.gradients).
Weights: humannerf_amd.seeded.seeded_state(default shapes, seed 0) with the view layers of
tests/viewdir_cases.view_tensors -- nothing but their seed is stored."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FULL_MAX = 32768


def main(ref):
    import torch
    sys.path.insert(0, REPO)
    from oracle import make_golden
    make_golden.REF = ref
    cfg, create_network = make_golden.import_reference()
    from humannerf_amd.seeded import default_shapes, seeded_state
    from tests import heads_train_cases as hc
    from tests import viewdir_cases as vc
    from tests.test_grad_oracle import compare_exact, grad_frame, reference_loss
    torch.set_num_threads(8)
    base = seeded_state(default_shapes(), seed=0)
    cfg.canonical_mlp.view_dir = True
    cfg.canonical_mlp.view_embed = 'mlp'
    cfg.canonical_mlp.multires_dir = vc.BANDS
    cfg.perturb, cfg.ignore_non_rigid_motions = 0.0, False

    def network(state, camera_only, train=False):
        cfg.canonical_mlp.view_dir_camera_only = camera_only
        net = create_network()
        assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: v.shape for k, v in state.items()}
        net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
        return net.train() if train else net.eval()

    # (head_id as oracle/make_golden.py passes it to the single-head reference: its _apply_mlp_kernals indexes it)
    tensors = lambda fr: dict({k: torch.from_numpy(np.ascontiguousarray(fr[k])) for k in vc.FRAME_KEYS},
                              head_id=torch.tensor(-1))

    # ---- the class alone, and the frame for both settings
    state = vc.view_state(base)
    rs = np.random.RandomState(6)
    xyz = rs.uniform(-1.3, 1.3, (vc.N_POINTS, 3)).astype(np.float32)
    dirs = (rs.standard_normal((vc.N_POINTS, 3)) * rs.uniform(0.2, 5.0, (vc.N_POINTS, 1))).astype(np.float32)
    from oracle import oracle
    pe = oracle.fourier_pe(torch.from_numpy(xyz), 10)
    save = {'pe': pe.numpy(), 'dirs': dirs, 'view_seed': np.int64(vc.VIEW_SEED), 'bands': np.int64(vc.BANDS),
            'n_rays': np.int64(vc.N_RAYS), 'S': np.int64(vc.FIXTURE_S)}
    cfg.N_samples = vc.FIXTURE_S
    fr = vc.fixture_frame(os.path.join(HERE, 'golden'))
    frames = []
    for camera_only in (False, True):
        net = network(state, camera_only)
        with torch.no_grad():
            if not camera_only:
                dir_embed = net.dir_embed_fn(torch.nn.functional.normalize(torch.from_numpy(dirs)))
                save['cls_raw'] = net.cnl_mlp(pos_embed=pe, dir_embed=dir_embed).numpy()
            frames.append(net(**tensors(fr), iter_val=1e7))
    for k in ('rgb', 'alpha', 'depth'):
        save[k] = np.stack([o[k].numpy() for o in frames])
    print('raw |max|', np.abs(save['cls_raw']).max(axis=0), 'alpha mean', save['alpha'].mean(axis=1),
          'max |rgb(camera_only) - rgb|', np.abs(save['rgb'][1] - save['rgb'][0]).max())

    # ---- gradients on the grad_s64 case
    with open(os.path.join(HERE, 'golden', 'meta.json')) as f:
        meta = json.load(f)['grad_s64']
    cfg.N_samples = meta['N_samples']
    gstate = vc.view_state(base, sigma_scale=vc.TRAIN_SIGMA_SCALE)
    gfr = vc.with_camera_row(grad_frame(meta))
    assert gfr['rays'].shape[1] == meta['n_rays']
    lw = hc.head_loss_weights(meta['n_rays'])[0]
    net = network(gstate, False, train=True)
    out = net(**tensors(gfr), iter_val=meta['iter_val'])
    loss = reference_loss(out, torch.from_numpy(lw))
    loss.backward()
    save['loss'] = np.float32(float(loss.detach()))
    grads = {}
    for k, p in net.named_parameters():
        g = p.grad
        grads[k] = np.zeros(tuple(p.shape), np.float32) if g is None else g.numpy().copy()
        save['norm/' + k] = np.float32(0.0 if g is None else g.norm().item())
        if g is not None and g.numel() <= FULL_MAX:
            save['grad/' + k] = g.numpy().copy()
        elif g is not None:
            save['head/' + k] = g.reshape(-1)[:4096].numpy().copy()
    exact, loss64 = vc.gradients(gstate, gfr, lw, iter_val=meta['iter_val'], N_samples=meta['N_samples'])
    stats = compare_exact(grads, exact, rel_norm=1.0, cos_min=0.0)
    save['noise_floor'] = np.float32(stats['worst_rel_norm_err'][0])
    save['noise_floor_cos'] = np.float64(stats['worst_cosine'][0])
    path = os.path.join(HERE, 'golden', 'viewdir.npz')
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path), 'bytes; loss', save['loss'], 'fp64 loss', loss64, 'fp32 reference vs fp64:', stats)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
