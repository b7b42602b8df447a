"""View-dependent colour (canonical_mlp.view_dir behind cfg.amd.view_dir), host side: the opt-in matrix, the reference's
parameter names, the fold against the reference's own class and the layered fp64 twin (tests/viewdir_cases.py), the C ABI
group, fixed_view's rules and the camera directions of the datasets.  No GPU."""
import os

import numpy as np
import pytest
import torch

import viewdir_cases as vc


def _config(opt_in=True, **other):
    """The default configuration with canonical_mlp.view_dir = True, cfg.amd.view_dir = ``opt_in`` and ``other``
    ('a__b' = value) on top."""
    from humannerf_amd.config import get_cfg_defaults
    c = get_cfg_defaults()
    c.canonical_mlp.view_dir = True
    c.amd.view_dir = opt_in
    for path, val in other.items():
        cur, parts = c, path.split('__')
        for p in parts[:-1]:
            if p not in cur:
                cur[p] = {}
            cur = cur[p]
        cur[parts[-1]] = val
    return c


@pytest.fixture()
def view_cfg():
    """cfg with view-dependent colour on (4 bands) for the test's duration; yields cfg."""
    from humannerf_amd.config import cfg
    keep = {k: cfg.canonical_mlp.get(k) for k in ('view_dir', 'view_embed', 'multires_dir', 'view_dir_camera_only')}
    keep_amd = cfg.amd.get('view_dir')
    cfg.canonical_mlp.view_dir, cfg.canonical_mlp.view_embed, cfg.canonical_mlp.multires_dir = True, 'mlp', vc.BANDS
    cfg.canonical_mlp.view_dir_camera_only = False
    cfg.amd.view_dir = True
    try:
        yield cfg
    finally:
        for k, v in keep.items():
            if v is None:
                cfg.canonical_mlp.pop(k, None)
            else:
                cfg.canonical_mlp[k] = v
        if keep_amd is None:
            cfg.amd.pop('view_dir', None)
        else:
            cfg.amd.view_dir = keep_amd


def test_opt_in_matrix():
    from humannerf_amd.network import check_config_is_built, view_dir_bands
    with pytest.raises(NotImplementedError, match=r'view_dir.*cfg\.amd\.view_dir'):
        check_config_is_built(_config(opt_in=False))                 # refused as before, and the option is named
    check_config_is_built(_config())
    assert view_dir_bands(_config()) == 4 and view_dir_bands(_config(opt_in=False)) == 0
    from humannerf_amd.config import get_cfg_defaults
    assert view_dir_bands(get_cfg_defaults()) == 0
    for camera_only in (False, True):
        check_config_is_built(_config(canonical_mlp__view_dir_camera_only=camera_only))
    for L in (1, 10):
        c = _config(canonical_mlp__multires_dir=L)
        check_config_is_built(c)
        assert view_dir_bands(c) == L
    refused = [(_config(canonical_mlp__multihead={'enable': True, 'head_depth': 1}, multihead={'head_num': 4}), 'view_dir'),
               (_config(canonical_mlp__view_embed='vocab'), 'vocab'),
               (_config(canonical_mlp__pose_color='direct'), 'pose_color'),
               (_config(canonical_mlp__pose_color='ao'), 'pose_color'),
               (_config(canonical_mlp__multires_dir=0), 'multires_dir'),
               (_config(canonical_mlp__multires_dir=11), 'multires_dir'),
               (_config(canonical_mlp__multires_dir=4.0), 'multires_dir'),
               (_config(canonical_mlp__multires_dir=True), 'multires_dir')]
    for c, key in refused:
        with pytest.raises(NotImplementedError, match=key):
            check_config_is_built(c)
    # the opt-in alone selects nothing
    c = get_cfg_defaults()
    c.amd.view_dir = True
    check_config_is_built(c)
    assert view_dir_bands(c) == 0


@pytest.fixture()
def view_net(view_cfg, seeded_params):
    from humannerf_amd.network import Network
    net = Network()
    state = vc.view_state(seeded_params)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return net.eval(), state


def test_strict_load_of_a_reference_shaped_state(view_cfg, seeded_params):
    """The reference's names and shapes (the fixture generator asserts the same table against the reference's own
    state_dict), no output_linear; nn.Linear's default initialisation on the four layers."""
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import view_shapes
    torch.manual_seed(3)
    net = Network()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert shapes == {k: tuple(v) for k, v in view_shapes(vc.BANDS).items()}
    assert not any('.output_linear.' in k for k in shapes)
    assert shapes['cnl_mlp.module.output_linear_rgb_2.0.weight'] == (256, 256 + 27)
    # default initialisation: U(+-1/sqrt(fan_in)) for weight and bias, biases not zeroed
    for name, fan_in in (('output_linear_density.0', 256), ('output_linear_rgb_1.0', 256),
                         ('output_linear_rgb_2.0', 283), ('output_linear_rgb_2.1', 256)):
        w, b = net.state_dict()[vc.P + name + '.weight'], net.state_dict()[vc.P + name + '.bias']
        bound = 1.0 / np.sqrt(fan_in)
        assert float(w.abs().max()) <= bound and float(b.abs().max()) <= bound and float(b.abs().max()) > 0
        if w.numel() > 1000:
            assert float(w.abs().max()) > 0.98 * bound
    state = vc.view_state(seeded_params)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_params.items()}, strict=True)
    with pytest.raises(RuntimeError, match='view branch'):
        net.cnl_mlp.module.linears()


def test_new_parameters_fall_in_the_canonical_group(view_net):
    """train.build_optimizer routes by name substring: the four layers, like the trunk, match none of cfg.train.lr_* and
    train at the base rate, one group per tensor named by its key."""
    from humannerf_amd.config import cfg
    from humannerf_amd.train import build_optimizer
    net, _ = view_net
    groups = {g['name']: g for g in build_optimizer(net).param_groups}
    for layer in vc.VIEW_LAYERS:
        for part in ('weight', 'bias'):
            g = groups[vc.P + layer + '.' + part]
            assert g['lr'] == cfg.train.lr and len(g['params']) == 1
    assert groups['cnl_mlp.module.pts_linears.0.weight']['lr'] == cfg.train.lr


def test_fold_matches_the_reference_class_and_the_layered_twin(view_net, golden_dir):
    """raw = [A ; Wd] h + [c ; bd] + (B e(d), 0) against the reference's CanonicalMLP(view_dir=True) (cls_raw of the
    fixture) and the layered fp64 twin.
      * The fold itself, in fp64, is within 1e-12 (relative to the largest raw value) of the twin.
      * The folded head -- built in fp64, rounded once, applied in fp32 -- is no farther from the fp64 branch than the
        reference's own arithmetic, the three fp32 layers, is: both on the SAME fp32 trunk output h, so that the
        trunk's eight fp32 layers (common to both, and larger than either head's error) do not blur the comparison.
      * End to end in fp32 (the oracle's fp32 trunk, then the folded head) it stays within the bound the reference's own
        fp32 output is held to against the twin, 1e-5 of the largest raw value."""
    from humannerf_amd.network import fold_view_branch, view_embedding
    from oracle import oracle
    net, state = view_net
    g = np.load(os.path.join(golden_dir, 'viewdir.npz'))
    pe, dirs = torch.from_numpy(g['pe']), torch.from_numpy(g['dirs'])
    twin = vc.canonical_view_raw(vc.t64(state, 'cnl_mlp'), pe.double(), dirs.double()).numpy()
    scale = np.abs(twin).max()
    assert np.abs(g['cls_raw'] - twin).max() <= 1e-5 * scale        # (the twin restates the reference's class)

    def trunk(dtype):                                                # the trunk output h from the oracle
        st = {k: torch.as_tensor(v).to(dtype) for k, v in state.items() if k.startswith('cnl_mlp')}
        st[vc.P + 'output_linear.0.weight'] = torch.zeros(1, 256, dtype=dtype)
        st[vc.P + 'output_linear.0.bias'] = torch.zeros(1, dtype=dtype)
        hidden = []
        oracle.canonical_mlp(st, pe.to(dtype), hidden)
        return hidden[-1]

    def layered(h, d):                                               # the reference's three layers + density, in h's dtype
        st = {k: torch.as_tensor(v).to(h.dtype) for k, v in state.items() if k.startswith('cnl_mlp')}
        L = vc.VIEW_LAYERS
        feat = torch.cat([oracle._lin(st, vc.P + L[1], h), vc.embed(d)], dim=1)
        return torch.cat([oracle._lin(st, vc.P + L[3], oracle._lin(st, vc.P + L[2], feat)), oracle._lin(st, vc.P + L[0], h)], 1)

    layers = net.cnl_mlp.module.view_layers()
    hw, hb, B = fold_view_branch(*layers, dtype=torch.float64)
    e64 = view_embedding(dirs.double(), vc.BANDS)
    assert torch.equal(e64, vc.embed(dirs.double()))
    raw64 = trunk(torch.float64) @ hw.t() + hb
    raw64[:, :3] += e64 @ B.t()
    assert np.abs(raw64.detach().numpy() - twin).max() <= 1e-12 * scale
    for got, want in zip((hw, hb, B), vc.fold_parts(state)):
        assert np.abs(got.detach().numpy() - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    # inference: folded in fp64, rounded once, applied in fp32
    w32, b32, B32, zero3 = net._view_fold()
    assert w32.dtype == b32.dtype == B32.dtype == torch.float32 and not w32.requires_grad and float(zero3.abs().sum()) == 0
    assert torch.equal(w32, hw.float()) and torch.equal(B32, B.float())

    def folded(h, d):
        raw = h @ w32.t() + b32
        raw[:, :3] += view_embedding(d, vc.BANDS) @ B32.t()
        return raw
    h32 = trunk(torch.float64).float()
    exact = layered(h32.double(), dirs.double())
    ref_dist = float((layered(h32, dirs).double() - exact).abs().max())
    fold_dist = float((folded(h32, dirs).double() - exact).abs().max())
    e2e = np.abs(folded(trunk(torch.float32), dirs).numpy().astype(np.float64) - twin).max()
    print('on one fp32 h: max |folded fp32 - fp64|', fold_dist, '| the reference\'s three fp32 layers', ref_dist,
          '| end to end in fp32', e2e, '| raw scale', scale)
    assert fold_dist <= ref_dist
    assert e2e <= 1e-5 * scale
    # training: the same function in fp32 under autograd reaches the four layers
    hw_t, hb_t, B_t = fold_view_branch(*layers)
    (hw_t.sum() + hb_t.sum() + B_t.sum()).backward()
    assert all(l.weight.grad is not None and l.bias.grad is not None for l in layers)
    assert float((hw_t.detach() - w32).abs().max()) <= 1e-5 * float(w32.abs().max())


def test_fold_is_kept_by_the_raw_parameters(view_net):
    net, _ = view_net
    first = net._view_fold()
    assert net._view_fold() is first                                 # (kept: the same tuple)
    with torch.no_grad():
        net.cnl_mlp.module.output_linear_rgb_2[1].weight.mul_(2.0)   # an in-place write autograd knows of
    second = net._view_fold()
    assert second is not first and torch.allclose(second[2], 2.0 * first[2], rtol=1e-6, atol=0)
    net.weights_changed()
    assert 'view_fold' not in net._kept
    with torch.no_grad():
        net.cnl_mlp.module.pts_linears[0].weight.add_(1.0)           # the trunk is not the fold's business
    third = net._view_fold()
    assert net._view_fold() is third


def test_view_group_is_bound_like_the_normals_group():
    from humannerf_amd import _lib
    assert 'view' in _lib.OPEN_GROUPS and _lib.OPEN_GROUPS['view'][0] == 'hnrf_view.h'
    assert len(_lib.SIGNATURES) == 88
    names = {'hnrf_view_bias_fwd', 'hnrf_view_bias_bwd', 'hnrf_view_bias_bwd_workspace_bytes', 'hnrf_composite_view_fwd',
             'hnrf_composite_view_bwd', 'hnrf_render_frame_view_fwd'}
    assert set(_lib.VIEW_SIGNATURES) == names and not names & set(_lib.SIGNATURES)
    lib = _lib.load_view()
    assert lib.hnrf_abi_version() == 13
    for n in names:
        assert getattr(lib, n).argtypes is not None
    assert lib.hnrf_view_bias_bwd_workspace_bytes(6144, 4) == 8192      # 24 slices x 28 columns x 3 floats, to 256 bytes
    assert lib.hnrf_view_bias_bwd_workspace_bytes(6144, 11) == 0 and lib.hnrf_view_bias_bwd_workspace_bytes(-1, 4) == 0

    class Old:                                                       # a library of ABI 13 built before the header
        pass
    with pytest.raises(_lib.HnrfError, match='view-dependent colour'):
        _lib.load_view(Old())


def test_fixed_view_rules(view_net, monkeypatch):
    """fixed_view folds B e(d0) into the colour bias of the packed image; colour without a ray and without a direction
    raises; density-only consumers and forward's own image need none."""
    from humannerf_amd import ops
    from humannerf_amd.network import Network
    net, state = view_net
    packs = []

    def fake_pack(W, B, mode, out=None):
        packs.append((W, B))
        return torch.zeros(4)
    monkeypatch.setattr(ops, 'canonical_pack', fake_pack)
    with pytest.raises(RuntimeError, match='fixed_view'):
        net._canonical_packed('fixed')
    with pytest.raises(RuntimeError, match='fixed_view'):
        net.vertex_colors(torch.zeros(2, 3))
    plain = net._canonical_packed()                                  # density only: no direction needed
    assert net._canonical_packed('ray') is plain and len(packs) == 1
    hw, hb, B, _ = net._view_fold()
    assert len(packs[0][0]) == 9 and packs[0][0][8] is hw and torch.equal(packs[0][1][8], hb)
    d0 = (0.3, -2.0, 1.1)
    assert net.fixed_view(d0) is net
    fixed = net._canonical_packed('fixed')
    assert fixed is not plain and len(packs) == 2
    want = hb.double().clone()
    want[:3] += B.double() @ vc.embed(torch.tensor(d0, dtype=torch.float64))
    assert float((packs[1][1][8].double() - want).abs().max()) <= 2e-7 * float(want.abs().max())
    assert torch.equal(packs[1][1][8][3], hb[3])                     # density untouched
    assert net._canonical_packed('fixed') is fixed and net._canonical_packed('ray') is plain and len(packs) == 2
    net.fixed_view((0.0, 0.0, 1.0))                                  # another direction: another image
    assert net._canonical_packed('fixed') is not fixed and len(packs) == 3
    net.fixed_view(None)
    with pytest.raises(RuntimeError, match='fixed_view'):
        net._canonical_packed('fixed')
    for bad in ((1.0, 2.0), (float('nan'), 0.0, 1.0)):
        with pytest.raises(ValueError):
            net.fixed_view(bad)
    # bake keys: the baked renderer's grid is keyed without a direction, a direct bake with one
    assert net._view_key('ray') == (None,) and net._view_key('fixed') == (None,)
    net.fixed_view(d0)
    assert net._view_key('fixed') == (d0,) and net._view_key('ray') == (None,)


def test_fixed_view_needs_a_view_branch():
    from humannerf_amd.network import Network
    net = Network()
    assert net.view_bands == 0 and net._view_key('fixed') == ()
    with pytest.raises(ValueError, match='view branch'):
        net.fixed_view((0.0, 0.0, 1.0))
    assert net.fixed_view(None) is net


def test_dataset_third_row_is_the_camera_direction(view_cfg, golden_dir):
    """With view_dir and view_dir_camera_only the third row of a train / movement frame's rays is the reference's
    rays_d_camera (train.py:562-565): the directions under the extrinsics BEFORE apply_global_tfm_to_camera, for the same
    pixels -- i.e. row 1 turned by R_before^T R_after.  Freeview and tpose frames keep [o, d, d]."""
    from humannerf_amd import dataset, scene
    subj = dataset.Subject(os.path.join(golden_dir, 'subject_synth'))
    idx = 1
    name = subj.framelist[idx]
    info, cam = subj.mesh_infos[name], subj.cameras[name]
    assert float(np.abs(info['Rh']).max()) > 0.1                     # (a frame whose root is turned: Rh != 0)
    H, W = subj.image_size(name)
    plain = subj.movement_frame(idx, host_rays=True, image_size=(H, W))
    assert np.array_equal(plain['rays'][2], plain['rays'][1])        # without camera_only: as before
    view_cfg.canonical_mlp.view_dir_camera_only = True
    assert dataset.view_camera_only()
    fr = subj.movement_frame(idx, host_rays=True, image_size=(H, W))
    assert np.array_equal(fr['rays'][:2], plain['rays'][:2]) and np.array_equal(fr['ray_mask'], plain['ray_mask'])
    K = cam['intrinsics'][:3, :3].copy()
    K[:2] *= view_cfg.get('resize_img_scale', 1.0)
    E0 = np.asarray(cam['extrinsics'])
    want = scene.get_rays_from_KRT(H, W, K, E0[:3, :3], E0[:3, 3])[1].reshape(-1, 3)[fr['ray_mask']].astype(np.float32)
    assert np.array_equal(fr['rays'][2], want)
    E1 = dataset.apply_global_tfm_to_camera(E0, info['Rh'].astype('float32'), info['Th'].astype('float32'))
    M = E0[:3, :3].astype(np.float64).T @ E1[:3, :3].astype(np.float64)
    assert np.allclose(M, dataset.camera_turn(E0, E1))
    assert np.abs(fr['rays'][2] - fr['rays'][1].astype(np.float64) @ M.T).max() <= 1e-6
    assert np.abs(fr['rays'][2] - fr['rays'][1]).max() > 1e-3        # it is another direction on this frame
    # the camera-only movement frame carries the turn for the device generator
    cam_fr = subj.movement_frame(idx, image_size=(H, W))
    assert 'rays' not in cam_fr and np.allclose(cam_fr['camera_turn'], M, atol=1e-7)
    # a training item: the same selection in all three rows
    np.random.seed(0)
    item = subj.train_frame(idx, bgcolor=[0, 0, 0])
    assert item['rays'].shape[0] == 3
    assert np.abs(item['rays'][2] - item['rays'][1].astype(np.float64) @ M.T).max() <= 1e-6
    # freeview and tpose keep [o, d, d] (tpose.py of the reference)
    for other in (subj.freeview_frame(1, 8, host_rays=True, image_size=(H, W)), subj.tpose_frame(1, 8, host_rays=True)):
        assert np.array_equal(other['rays'][2], other['rays'][1])
    assert 'camera_turn' not in subj.freeview_frame(1, 8, image_size=(H, W))
    view_cfg.canonical_mlp.view_dir_camera_only = False
    assert 'camera_turn' not in subj.movement_frame(idx, image_size=(H, W))


def test_forward_refusals_on_the_host(view_net, golden_dir):
    """camera-only without a third row, and early ray termination, are refused by name before any kernel is reached (the
    weight volume is injected, so nothing here needs a device)."""
    from humannerf_amd.config import cfg
    net, _ = view_net
    fr = vc.fixture_frame(golden_dir)
    data = {k: torch.from_numpy(np.ascontiguousarray(fr[k])) for k in vc.FRAME_KEYS}
    stop = RuntimeError('reached the kernels')

    def no_kernels(*a, **k):
        raise stop
    net._canonical_packed = lambda colour=None: torch.zeros(4)
    net._nonrigid_packed = lambda cond: torch.zeros(4)
    net._weight_volume = lambda priors: torch.zeros(25, 32, 32, 32)
    net._forward_frame = no_kernels
    import humannerf_amd.network as nw
    keep_basis = nw.motion_basis
    nw.motion_basis = lambda *a, **k: (torch.zeros(24, 3, 3), torch.zeros(24, 3))
    keep = cfg.N_samples, cfg.perturb, cfg.amd.get('term_eps', 0.0), cfg.amd.get('diagnostics', True)
    cfg.N_samples, cfg.perturb = vc.FIXTURE_S, 0.0
    try:
        with torch.no_grad():
            cfg.canonical_mlp.view_dir_camera_only = True
            two = dict(data, rays=data['rays'][:2].contiguous())
            with pytest.raises(ValueError, match='view_dir_camera_only'):
                net(**two)
            cfg.canonical_mlp.view_dir_camera_only = False
            cfg.amd.term_eps, cfg.amd.diagnostics = 1e-3, False
            with pytest.raises(NotImplementedError, match='term_eps'):
                net(**data)
    finally:
        nw.motion_basis = keep_basis
        cfg.N_samples, cfg.perturb, cfg.amd.term_eps, cfg.amd.diagnostics = keep
        cfg.canonical_mlp.view_dir_camera_only = False
