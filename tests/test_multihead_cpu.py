"""The multi-head canonical MLP without a GPU: which configurations are built, the module tree and a strict load of a
reference-shaped state, head selection and the pack keys, the exported entries, and the fp64 twin of
tests/multihead_cases.py against the reference's outputs (tests/golden/multihead.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import multihead_cases as mc


def _config(enable=True, head_num=None, head_depth=None, **other):
    from humannerf_amd.config import get_cfg_defaults
    c = get_cfg_defaults()
    node = {'enable': enable}
    if head_depth is not None:
        node['head_depth'] = head_depth
    c.canonical_mlp.multihead = node
    if head_num is not None:
        c.multihead = {'head_num': head_num, 'split': 'view'}
    for path, val in other.items():
        cur, parts = c, path.split('__')
        for p in parts[:-1]:
            if p not in cur:
                cur[p] = {}
            cur = cur[p]
        cur[parts[-1]] = val
    return c


def test_built_and_unbuilt_configurations():
    from humannerf_amd.network import canonical_head_num, check_config_is_built
    for H in range(2, 9):
        c = _config(head_num=H, head_depth=1)
        check_config_is_built(c)
        assert canonical_head_num(c) == H
    check_config_is_built(_config(head_num=4))                       # head_depth absent: the reference's default, 1
    check_config_is_built(_config(enable=False, head_num=1))         # the reference's default nodes
    assert canonical_head_num(_config(enable=False, head_num=4)) == 0
    refused = [(_config(), 'head_num'),                              # no multihead node
               (_config(head_num=1), 'head_num'), (_config(head_num=9), 'head_num'), (_config(head_num=0), 'head_num'),
               (_config(head_num=2.0), 'head_num'), (_config(head_num=True), 'head_num'),
               (_config(head_num=4, head_depth=2), 'head_depth'),
               (_config(head_num=4, canonical_mlp__view_dir=True), 'view_dir'),
               (_config(head_num=4, canonical_mlp__pose_color='direct'), 'pose_color'),
               (_config(head_num=4, non_rigid_motion_mlp__multihead__enable=True), r'non_rigid_motion_mlp\.multihead\.enable')]
    for c, key in refused:
        with pytest.raises(NotImplementedError, match=key):
            check_config_is_built(c)


@pytest.fixture(scope='module')
def net3():
    """A 3-head Network on the CPU; the configuration is restored at once (the module tree is fixed at construction)."""
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network
    keep = (cfg.get('multihead'), cfg.canonical_mlp.get('multihead'))
    cfg.canonical_mlp.multihead = {'enable': True, 'head_depth': 1}
    cfg.multihead = {'head_num': 3}
    try:
        return Network()
    finally:
        for node, key, val in ((cfg, 'multihead', keep[0]), (cfg.canonical_mlp, 'multihead', keep[1])):
            if val is None:
                node.pop(key)
            else:
                node[key] = val


def test_state_dict_and_strict_load(net3, seeded_params):
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes
    sd = net3.state_dict()
    want = dict(default_shapes())
    want[mc.W_KEY], want[mc.B_KEY] = (12, 256), (12,)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want     # the reference's key names (mlp_rgb_sigma.py:114-115)
    assert net3.head_num == 3 and Network().head_num == 0
    # the initialiser of the single head (_init_sequence: no activation follows, gain 1) on the (4H, 256) tensor, zero bias
    bound = np.sqrt(6.0 / (12 + 256))
    w = sd[mc.W_KEY]
    assert 0.9 * bound < float(w.abs().max()) <= bound and float(sd[mc.B_KEY].abs().max()) == 0.0
    state = mc.multihead_state(seeded_params, 3)
    net3.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    assert torch.equal(net3.state_dict()[mc.W_KEY], torch.from_numpy(state[mc.W_KEY]))
    with pytest.raises(RuntimeError, match='size mismatch'):
        Network().load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)


def test_head_selection_and_pack_keys(net3, monkeypatch):
    """Which rows are packed under which key: the selected head as a single-head image of its four rows, -1 as the
    all-heads image, the head in the key; no selection raises."""
    from humannerf_amd import ops
    calls = []

    def single(ws, bs, mode='f32', out=None):
        calls.append(('single', tuple(ws[8].shape), ws[8].data_ptr(), bs[8].data_ptr(), out))
        return torch.zeros(4)

    def heads(ws, bs, n_heads, mode='f32', out=None):
        calls.append(('heads', tuple(ws[8].shape), n_heads, out))
        return torch.zeros(4)

    monkeypatch.setattr(ops, 'canonical_pack', single)
    monkeypatch.setattr(ops, 'canonical_heads_pack', heads)
    net3._drop(lambda e: e.packed is not None)
    net3.select_head(None)
    with pytest.raises(RuntimeError, match='select_head'):
        net3._canonical_packed()
    W, b = net3.cnl_mlp.module.output_linear[0].weight, net3.cnl_mlp.module.output_linear[0].bias
    images = {}
    for h in (0, 2, 1):
        assert net3.select_head(h) is net3
        images[h] = net3._canonical_packed()
        kind, shape, wp, bp, out = calls[-1]
        assert (kind, shape, out) == ('single', (4, 256), None)
        assert wp == W.data_ptr() + 4 * h * 256 * 4 and bp == b.data_ptr() + 4 * h * 4
        assert net3._kept[net3._pack_last].key == (net3._mlp_mode(), h) and net3._kept[net3._pack_last].packed is images[h]
    n = len(calls)
    for h in (0, 1, 2):                                             # every head keeps its image: nothing is packed again
        assert net3.select_head(h)._canonical_packed() is images[h]
    assert len(calls) == n
    net3._head = -1                                                 # what forward(head_id=-1) sets for the frame
    every = net3._canonical_packed()
    assert calls[-1][:3] == ('heads', (12, 256), 3) and net3._kept[net3._pack_last].key[1] == -1
    assert all(every is not v for v in images.values())
    with torch.no_grad():
        W.add_(0)                                                   # a weight update: the key's versions change
    net3.select_head(1)
    assert net3._canonical_packed() is not None and calls[-1][0] == 'single' and calls[-1][4] is images[1]   # (its buffer)
    assert len(calls) == n + 2
    for bad in (3, -1, 17):
        with pytest.raises(ValueError):
            net3.select_head(bad)
    net3.select_head(None)
    # forward's head_id: an int or a tensor of one element, read on the host
    assert net3._resolve_head(2) == 2 and net3._resolve_head(torch.tensor(-1)) == -1
    assert net3._resolve_head(torch.tensor([[1]])) == 1
    for bad in (3, -2, torch.tensor(5)):
        with pytest.raises(ValueError):
            net3._resolve_head(bad)
    with pytest.raises(RuntimeError, match='head_id'):
        net3._resolve_head(None)
    from humannerf_amd.network import Network
    with pytest.raises(ValueError):
        Network().select_head(0)


def test_training_is_refused(net3):
    from humannerf_amd.train import Trainer
    with pytest.raises(NotImplementedError, match='inference only'):
        Trainer(net3)
    fr = {k: None for k in ('rays', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors')}
    with pytest.raises(NotImplementedError, match='inference only'):
        net3(**fr, head_id=0)                                       # grad mode, parameters that require grad


def test_new_entries_are_exported():
    from humannerf_amd import _lib
    names = ['hnrf_canonical_heads_fwd', 'hnrf_canonical_heads_fwd_sparse', 'hnrf_canonical_heads_pack',
             'hnrf_render_frame_heads_fwd', 'hnrf_render_frame_heads_workspace_bytes']
    assert sorted(_lib.HEADS_SIGNATURES) == names
    assert not set(_lib.HEADS_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.CLOUD_SIGNATURES) | set(_lib.VIDEO_SIGNATURES)
                                             | set(_lib.SEGMENT_SIGNATURES) | set(_lib.GEOMETRY_SIGNATURES))
    vp, i64, i, sz, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
    assert _lib.HEADS_SIGNATURES['hnrf_canonical_heads_pack'] == (i, [vp, vp, i, i, vp, vp])
    assert _lib.HEADS_SIGNATURES['hnrf_canonical_heads_fwd_sparse'] == (i, [vp, vp, i, i64, i, vp, vp, vp, vp])
    assert _lib.HEADS_SIGNATURES['hnrf_render_frame_heads_workspace_bytes'] == (sz, [i64, i, i])
    assert _lib.HEADS_SIGNATURES['hnrf_render_frame_heads_fwd'] == (
        i, [vp] * 14 + [i, f, i64, i, i, i, i64, i, vp, sz] + [vp] * 15)
    lib = _lib.load_heads()
    for name in names:
        assert hasattr(lib, name)
    assert lib.hnrf_abi_version() == 13 and len(_lib.SIGNATURES) == 88
    one = lib.hnrf_render_frame_workspace_bytes(96, 16)
    assert lib.hnrf_render_frame_heads_workspace_bytes(96, 16, 3) == one + 3 * 96 * 16 * 16
    assert lib.hnrf_render_frame_heads_workspace_bytes(96, 16, 1) == 0 == lib.hnrf_render_frame_heads_workspace_bytes(96, 16, 9)
    # argument errors come back before anything touches a device
    assert lib.hnrf_canonical_heads_fwd(None, None, 0, 4, 3, None, None) == -1
    assert lib.hnrf_canonical_heads_pack(None, None, 9, 0, None, None) == -1 and b'n_heads' in lib.hnrf_last_error()


@pytest.fixture(scope='module')
def fixture_npz(golden_dir):
    path = os.path.join(golden_dir, 'multihead.npz')
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(golden_dir, 'eval_s64.npz'))
    g = np.load(path)
    assert int(g['head_seed']) == mc.HEAD_SEED and int(g['S']) == mc.FIXTURE_S
    return g


@pytest.mark.parametrize('H', mc.FIXTURE_HEADS)
def test_twin_head_layer_matches_reference_class(H, fixture_npz, seeded_params):
    """The reference's CanonicalMLP: its head_id = -1 list and its head_id = h outputs are the same numbers, and the fp64
    twin (the oracle on the head's sliced rows; all heads from one trunk) holds to them within the raw bound of
    tests/test_oracle_golden.py, 5e-4 of the largest raw."""
    g = fixture_npz
    every, each, pe = g['H%d/cls_all' % H], g['H%d/cls_each' % H], g['pe']
    assert every.shape == each.shape == (H, pe.shape[0], 4) and np.array_equal(every, each)
    state = mc.multihead_state(seeded_params, H)
    twin = mc.heads_raw64(state, pe=pe)
    top = max(1.0, np.abs(each).max())
    for h in range(H):
        assert np.abs(twin[h] - each[h]).max() <= 5e-4 * top, h
        if h in (0, H - 1):
            assert np.abs(mc.head_raw64(state, h, pe) - twin[h]).max() <= 1e-12 * top
    assert np.abs(each[0] - each[1]).max() > 1.0                    # the heads are different networks


@pytest.mark.parametrize('H', mc.FIXTURE_HEADS)
def test_twin_frame_matches_reference_network(H, fixture_npz, seeded_params, golden_frame):
    """Per-head compositing: the fp64 twin's frame of head h holds to the reference Network.forward(head_id=h) within the
    bound tests/test_oracle_golden.py uses for the fp64 oracle against the fp32 reference, rgb 5e-5
    (test_oracle_fp64_close_to_fp32; that file bounds no other key in fp64, alpha and depth are printed)."""
    g = fixture_npz
    n = int(g['n_rays'])
    fr = dict(golden_frame)
    fr['rays'], fr['near'], fr['far'] = golden_frame['rays'][:, :n], golden_frame['near'][:n], golden_frame['far'][:n]
    outs = mc.render_heads(mc.multihead_state(seeded_params, H), fr, mc.FIXTURE_S)
    for h in range(H):
        err = {k: np.abs(outs[h][k] - g['H%d/%s' % (H, k)][h]).max() for k in ('rgb', 'alpha', 'depth')}
        print('twin fp64 vs reference, H', H, 'head', h, ' '.join('%s %.1e' % kv for kv in err.items()))
        assert err['rgb'] < 5e-5, (h, err)
        # the twin's compositing, stated on its own: raw2outputs of the head's raw
        o = outs[h]
        again = mc.composite_heads64([o['_raw']], o['_mask'], o['_z_vals'], fr['rays'][1], o['xyz_on_rays'], fr['bgcolor'])[0]
        assert np.array_equal(again['rgb'], o['rgb']) and np.array_equal(again['alpha'], o['alpha'])
    assert np.abs(g['H%d/alpha' % H][0] - g['H%d/alpha' % H][1]).max() > 1e-2
