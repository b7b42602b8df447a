"""Training a multi-head canonical MLP, the parts that need no GPU: the opt-in switch cfg.amd.train_heads, the exported
entries and their refusals, the 'argmin' loss against a restatement of the reference's (trainer.py:124-160), and the
head_id of training items for the four forms of multihead.split."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch


@pytest.fixture()
def heads_cfg():
    """cfg of a 3-head run for the duration of a test (restored afterwards); yields cfg."""
    from humannerf_amd.config import cfg
    keep = (cfg.get('multihead'), cfg.canonical_mlp.get('multihead'), cfg.amd.get('train_heads'), cfg.get('test'),
            cfg.train.lossweights.clone())
    cfg.canonical_mlp.multihead = {'enable': True, 'head_depth': 1}
    cfg.multihead = {'head_num': 3}
    try:
        yield cfg
    finally:
        for node, key, val in ((cfg, 'multihead', keep[0]), (cfg.canonical_mlp, 'multihead', keep[1]),
                               (cfg.amd, 'train_heads', keep[2]), (cfg, 'test', keep[3])):
            if val is None:
                node.pop(key, None)
            else:
                node[key] = val
        cfg.train.lossweights = keep[4]


def test_switch_is_off_by_default_and_the_refusals_name_it(heads_cfg):
    from humannerf_amd.config import _DEFAULTS, amd_option
    from humannerf_amd.network import Network
    from humannerf_amd.train import Trainer
    assert _DEFAULTS['amd']['train_heads'] is False and amd_option('train_heads') is False
    net = Network()
    assert net.head_num == 3
    with pytest.raises(NotImplementedError, match='inference only') as e:
        Trainer(net)
    assert 'cfg.amd.train_heads' in str(e.value)
    fr = {k: None for k in ('rays', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors')}
    for head in (0, -1):
        with pytest.raises(NotImplementedError, match='inference only') as e:
            net(**fr, head_id=head)                                 # grad mode, parameters that require grad
        assert 'cfg.amd.train_heads' in str(e.value)
    heads_cfg.amd.train_heads = True
    tr = Trainer(net)                                               # accepted; sizes come from the parameters
    sizes = {tuple(p.shape) for g in tr.optimizer.param_groups for p in g['params']}
    assert (12, 256) in sizes and (12,) in sizes


def test_new_entries_are_exported_in_an_open_group():
    from humannerf_amd import _lib
    assert 'heads_train' in _lib.OPEN_GROUPS
    names = ['hnrf_canonical_heads_bwd', 'hnrf_canonical_heads_bwd_pack', 'hnrf_canonical_heads_bwd_packed_bytes',
             'hnrf_canonical_heads_fwd_train']
    assert sorted(_lib.HEADS_TRAIN_SIGNATURES) == names
    assert not set(names) & (set(_lib.SIGNATURES) | set(_lib.HEADS_SIGNATURES) | set(_lib.HEADS_SHARED_SIGNATURES))
    vp, i64, i, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    assert _lib.HEADS_TRAIN_SIGNATURES['hnrf_canonical_heads_fwd_train'] == (i, [vp, vp, i, i64, i, vp, vp, vp, vp, vp])
    assert _lib.HEADS_TRAIN_SIGNATURES['hnrf_canonical_heads_bwd_packed_bytes'] == (sz, [i, i])
    assert _lib.HEADS_TRAIN_SIGNATURES['hnrf_canonical_heads_bwd_pack'] == (i, [vp, i, i, vp, vp])
    assert _lib.HEADS_TRAIN_SIGNATURES['hnrf_canonical_heads_bwd'] == (i, [vp, vp, vp, vp, i, vp, i64, i, vp, vp, vp, vp])
    lib = _lib.load_heads_train()
    for name in names:
        assert hasattr(lib, name)
    assert lib.hnrf_abi_version() == 13 and len(_lib.SIGNATURES) == 88 and len(_lib.HEADS_SIGNATURES) == 5


def test_bad_head_counts_and_null_pointers_are_refused_before_any_launch():
    """No GPU is present when this runs: an entry that launched anything would fail differently (HNRF_E_LAUNCH)."""
    from humannerf_amd import _lib
    lib = _lib.load_heads_train()
    E_ARG = -1
    buf = (ctypes.c_float * 64)()                                   # a valid, 16-byte aligned host address: never read
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    ptrs9 = (ctypes.c_void_p * 9)(*[p] * 9)
    for H in (-1, 0, 1, 9, 64):
        assert lib.hnrf_canonical_heads_fwd_train(p, p, 0, 128, H, p, p, p, p, None) == E_ARG
        assert b'n_heads' in lib.hnrf_last_error()
        assert lib.hnrf_canonical_heads_bwd_pack(ptrs9, H, 0, p, None) == E_ARG
        assert b'n_heads' in lib.hnrf_last_error()
        assert lib.hnrf_canonical_heads_bwd(p, p, p, p, 0, None, 128, H, p, p, None, None) == E_ARG
        assert b'n_heads' in lib.hnrf_last_error()
        for mode in (0, 1):
            assert lib.hnrf_canonical_heads_bwd_packed_bytes(mode, H) == 0
    for mode in (0, 1):
        sizes = [lib.hnrf_canonical_heads_bwd_packed_bytes(mode, H) for H in range(2, 9)]
        assert len(set(sizes)) == 1 and sizes[0] > lib.hnrf_canonical_bwd_packed_bytes(mode) > 0
    assert lib.hnrf_canonical_heads_bwd_packed_bytes(2, 4) == 0     # (the f16-operand mode shares the 'f16x3' image)
    for k in range(4):                                              # xyz, packed, raw, pe_out: each null in turn
        args = [p, p, 0, 128, 3, p, p, p, p, None]
        args[(0, 1, 5, 6)[k]] = None
        assert lib.hnrf_canonical_heads_fwd_train(*args) == E_ARG and b'null' in lib.hnrf_last_error()
    for k in (0, 1, 2, 3, 8, 9):                                    # xyz, d_raw, relu_bits, packed, dZ, d_xyz
        args = [p, p, p, p, 0, None, 128, 3, p, p, None, None]
        args[k] = None
        assert lib.hnrf_canonical_heads_bwd(*args) == E_ARG and b'null' in lib.hnrf_last_error()
    assert lib.hnrf_canonical_heads_bwd(p, p, p, p, 1, None, 128, 3, p, p, None, None) == E_ARG      # split-f16 needs the bound
    assert lib.hnrf_canonical_heads_bwd(p, p, p, p, 2, p, 128, 3, p, p, None, None) == E_ARG         # f16 dZ needs the scales
    assert lib.hnrf_canonical_heads_bwd_pack(None, 3, 0, p, None) == E_ARG
    assert lib.hnrf_canonical_heads_bwd_pack(ptrs9, 3, 0, None, None) == E_ARG
    assert lib.hnrf_canonical_heads_fwd_train(p, p + 4, 0, 128, 3, p, p, p, p, None) == E_ARG        # misaligned image
    assert lib.hnrf_canonical_heads_fwd_train(p, p, 0, 0, 3, p, p, p, p, None) == 0                  # P = 0: nothing to do


def test_single_head_entries_refuse_what_they_refused_and_name_themselves():
    """The same table for hnrf_canonical_fwd_train, hnrf_canonical_bwd_pack and hnrf_canonical_bwd, which share their
    bodies with the _heads entries: the codes are those the library gave while each entry still had a body of its own,
    and the message names the entry that was called, never its twin.  No GPU: nothing may be launched."""
    from humannerf_amd import _lib
    lib = _lib.load_heads_train()
    E_ARG, E_UNSUPPORTED = -1, -2
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    ptrs9 = (ctypes.c_void_p * 9)(*[p] * 9)

    def refused(entry, code, *args, word=b''):
        assert getattr(lib, entry)(*args) == code, (entry, args)
        msg = lib.hnrf_last_error()
        assert msg.startswith(entry.encode() + b':') and word in msg, msg

    for k in (0, 1, 4, 5, 6, 7):                                    # xyz, packed, raw, pe_out, acts, relu_bits
        args = [p, p, 0, 128, p, p, p, p, None]
        args[k] = None
        refused('hnrf_canonical_fwd_train', E_ARG, *args, word=b'null pointer')
    for k in (0, 1, 2, 3, 7, 8):                                    # xyz, d_raw, relu_bits, packed, dZ, d_xyz
        args = [p, p, p, p, 0, None, 128, p, p, None, None]
        args[k] = None
        refused('hnrf_canonical_bwd', E_ARG, *args, word=b'null pointer')
    refused('hnrf_canonical_bwd_pack', E_ARG, None, 0, p, None, word=b'null pointer')
    refused('hnrf_canonical_bwd_pack', E_ARG, ptrs9, 0, None, None, word=b'null pointer')
    holed = (ctypes.c_void_p * 9)(*[p] * 9)
    holed[5] = None
    refused('hnrf_canonical_bwd_pack', E_ARG, holed, 0, p, None, word=b'null layer 5')
    # split-f16 without its bound (the single-head wording: no "over all planes"), f16 dZ without its scales
    refused('hnrf_canonical_bwd', E_ARG, p, p, p, p, 1, None, 128, p, p, None, None, word=b'>= max |d_raw|)')
    refused('hnrf_canonical_bwd', E_ARG, p, p, p, p, 2, p, 128, p, p, None, None, word=b'needs dz_amax')
    assert lib.hnrf_canonical_heads_bwd(p, p, p, p, 1, None, 128, 3, p, p, None, None) == E_ARG
    assert lib.hnrf_last_error().startswith(b'hnrf_canonical_heads_bwd:') and b'over all planes' in lib.hnrf_last_error()
    # a mode that is not built; two faults at once report the earlier check (null before mode, mode before alignment)
    refused('hnrf_canonical_fwd_train', E_UNSUPPORTED, p, p, 7, 128, p, p, p, p, None, word=b'mode 7 not built')
    refused('hnrf_canonical_bwd', E_UNSUPPORTED, p, p, p, p, 7, None, 128, p, p, None, None, word=b'mode 7 not built')
    refused('hnrf_canonical_bwd_pack', E_UNSUPPORTED, ptrs9, 2, p, None, word=b'mode 2 not built')
    refused('hnrf_canonical_fwd_train', E_ARG, None, p + 4, 7, 128, p, p, p, p, None, word=b'null pointer')
    refused('hnrf_canonical_fwd_train', E_UNSUPPORTED, p, p + 4, 7, 128, p, p, p, p, None, word=b'not built')
    refused('hnrf_canonical_bwd', E_ARG, p, p, p, p + 4, 1, None, 128, p, p, None, None, word=b'd_raw_amax')
    # misaligned images and buffers; negative P
    refused('hnrf_canonical_fwd_train', E_ARG, p, p + 4, 0, 128, p, p, p, p, None, word=b'16-byte aligned')
    refused('hnrf_canonical_fwd_train', E_ARG, p, p, 0, 128, p, p, p + 4, p, None, word=b'16-byte aligned')
    refused('hnrf_canonical_bwd', E_ARG, p, p, p, p + 4, 0, None, 128, p, p, None, None, word=b'16-byte aligned')
    refused('hnrf_canonical_fwd_train', E_ARG, p, p, 0, -1, p, p, p, p, None, word=b'bad P')
    refused('hnrf_canonical_bwd', E_ARG, p, p, p, p, 0, None, -1, p, p, None, None, word=b'bad P')
    # (the 16-byte check of the image is the _heads pack's alone; that the single-head pack makes none cannot be shown
    # here without letting it go on to a launch)
    refused('hnrf_canonical_heads_bwd_pack', E_ARG, ptrs9, 3, 0, p + 4, None, word=b'16-byte aligned')
    # P = 0: nothing to do, in every mode; these calls carry no n_heads
    for mode in (0, 1, 2):
        assert lib.hnrf_canonical_fwd_train(p, p, mode, 0, p, p, p, p, None) == 0
        assert lib.hnrf_canonical_bwd(p, p, p, p, mode, p, 0, p, p, p, None) == 0
    assert lib.hnrf_canonical_bwd(p, p, p, p, 0, None, 0, p, p, None, None) == 0
    for mode in (0, 1):
        assert lib.hnrf_canonical_bwd_packed_bytes(mode) > 0
    assert lib.hnrf_canonical_bwd_packed_bytes(2) == 0


# ---------------------------------------------------------------------------------------------------- 'argmin' loss
def reference_argmin_loss(rgbs, target, lossweights, selector, unselected):
    """trainer.py:124-160 restated line by line for mse / l1 terms (numpy, float64)."""
    lossweights = {k: v for k, v in lossweights.items() if v > 0}
    loss_names = list(lossweights.keys())
    def rebuild(rgb):
        losses = {}
        if 'mse' in loss_names:
            losses['mse'] = np.mean((rgb - target) ** 2)
        if 'l1' in loss_names:
            losses['l1'] = np.mean(np.abs(rgb - target))
        losses['lpips'] = 0
        return losses
    return_losses, criteria_head, selected_losses, unselected_losses = {}, [], [], []
    for hid, rgb in enumerate(rgbs):
        losses = rebuild(rgb)
        selected_losses.append([w * losses[k] for k, w in lossweights.items()])
        unselected_losses.append([w * losses[k] for k, w in unselected.items()])
        criteria_head.append(sum(w * losses[k] for k, w in selector.items() if w > 0))
        return_losses.update({loss_names[i] + '_head%d' % hid: selected_losses[-1][i] for i in range(len(loss_names))})
    best_head = int(np.argmin(criteria_head))
    train_losses = list(selected_losses[best_head])
    return_losses.update({loss_names[i]: train_losses[i] for i in range(len(loss_names))})
    return_losses['best_head'] = best_head
    for head_id in range(len(rgbs)):
        if head_id != best_head:
            train_losses += unselected_losses[head_id]
    return sum(train_losses), return_losses


def _images(order, seed=3):
    """target and three head images at distances from it that rank in ``order`` (0 = closest; equal ranks = equal images)."""
    rs = np.random.RandomState(seed)
    target = rs.uniform(0.2, 0.8, (2, 8, 8, 3))
    noise = rs.standard_normal(target.shape)
    return target, [target + 0.01 * (1 + o) * noise for o in order]


@pytest.mark.parametrize('case', ['first', 'last', 'tied', 'unselected', 'l1'])
def test_argmin_loss_matches_the_restated_reference(heads_cfg, case):
    from humannerf_amd.train import heads_image_loss
    order = {'first': (0, 1, 2), 'last': (2, 1, 0), 'tied': (1, 0, 0), 'unselected': (1, 0, 2), 'l1': (2, 0, 1)}[case]
    target, rgbs = _images(order)
    weights = {'lpips': 0.0, 'mse': 0.2, 'l1': 0.5 if case == 'l1' else 0.0}
    selector = {'lpips': 1.0, 'mse': 0.2, 'ssim': 0.0} if case != 'l1' else {'mse': 0.0, 'l1': 1.0}
    unselected = {'lpips': 0.0, 'mse': 0.05 if case == 'unselected' else 0.0}
    heads_cfg.train.lossweights = weights
    heads_cfg.multihead = {'head_num': 3, 'split': 'argmin',
                           'argmin_cfg': {'selector_criteria': selector, 'unselected_lossweights': unselected}}
    want_total, want = reference_argmin_loss(rgbs, target, weights, selector, unselected)
    assert want['best_head'] == {'first': 0, 'last': 2, 'tied': 1, 'unselected': 1, 'l1': 1}[case]
    leaves = [torch.from_numpy(r).requires_grad_(True) for r in rgbs]
    total, parts, best = heads_image_loss(leaves, torch.from_numpy(target))
    assert best == want['best_head'] == parts['best_head']
    assert sorted(parts) == sorted(want)
    for k, v in want.items():
        assert abs(float(parts[k]) - float(v)) <= 1e-12 * max(1.0, abs(float(v))), k
    assert abs(float(total) - float(want_total)) <= 1e-12
    total.backward()
    for h, leaf in enumerate(leaves):                               # zero unselected weights: a zero gradient, not None
        if h != best and unselected['mse'] == 0.0:
            assert leaf.grad is None or float(leaf.grad.abs().max()) == 0.0
        else:
            assert float(leaf.grad.abs().max()) > 0.0


def test_argmin_defaults_and_the_ssim_criterion(heads_cfg):
    from humannerf_amd.config import multihead_option
    from humannerf_amd.train import heads_image_loss
    assert multihead_option('split') == 'view'                      # cfg.multihead = {'head_num': 3}: the defaults fill in
    assert dict(multihead_option('argmin_cfg.selector_criteria')) == {'lpips': 1.0, 'mse': 0.2, 'ssim': 0.0}
    assert dict(multihead_option('argmin_cfg.unselected_lossweights')) == {'lpips': 0.0, 'mse': 0.0}
    heads_cfg.multihead = {'head_num': 3, 'argmin_cfg': {'selector_criteria': {'mse': 1.0, 'ssim': 0.5}}}
    target, rgbs = _images((0, 1, 2))
    with pytest.raises(NotImplementedError, match='selector_criteria.ssim'):
        heads_image_loss([torch.from_numpy(r) for r in rgbs], torch.from_numpy(target))


# ----------------------------------------------------------------------------------------------------- head_id
def test_head_id_of_training_items_for_the_four_splits(heads_cfg, golden_dir, tmp_path):
    from humannerf_amd import dataset
    subject = dataset.Subject(os.path.join(golden_dir, 'subject_synth'))
    names = list(subject.framelist)
    assert len(names) == 3
    # with the switch off items are what they were: no head_id, in either mode
    assert 'head_id' not in subject.train_frame(0, bgcolor=[0, 0, 0]) and 'head_id' not in subject.movement_frame(0, image_size=(64, 64))
    heads_cfg.amd.train_heads = True
    # 'view' (the default): the index of the frame's view among the sorted views; this subject has one camera
    assert [subject.train_frame(i, bgcolor=[0, 0, 0])['head_id'] for i in range(3)] == [0, 0, 0]
    assert dataset.parse_view_from_frame('frame_000008_view_03') == 3 and dataset.parse_view_from_frame('Camera_B4/000438') == 4
    views = dataset.HeadAssignment(['frame_000001_view_07', 'frame_000001_view_02', 'frame_000002_view_07', 'frame_000001'])
    assert views.views == [0, 2, 7]
    assert [views.train(n) for n in ('frame_000002_view_07', 'frame_000001_view_02', 'frame_000001')] == [2, 1, 0]
    heads_cfg.multihead = {'head_num': 3, 'split': 'argmin'}
    assert [subject.train_frame(i, bgcolor=[0, 0, 0])['head_id'] for i in range(3)] == [-1, -1, -1]
    heads_cfg.multihead = {'head_num': 3, 'split': 'random'}
    np.random.seed(11)
    got = [subject.head_assignment().train(names[0]) for _ in range(64)]
    np.random.seed(11)
    assert got == [int(np.random.randint(3)) for _ in range(64)] and set(got) == {0, 1, 2}
    assert 0 <= subject.train_frame(0, bgcolor=[0, 0, 0])['head_id'] < 3
    table = {names[0]: 2, names[1]: 0, names[2]: 1}
    path = tmp_path / 'heads.json'
    path.write_text(json.dumps(table))
    heads_cfg.multihead = {'head_num': 3, 'split': str(path)}
    assert [subject.train_frame(i, bgcolor=[0, 0, 0])['head_id'] for i in range(3)] == [2, 0, 1]
    heads_cfg.multihead = {'head_num': 3, 'split': 'no_such_split'}
    with pytest.raises(ValueError, match='multihead.split'):
        subject.train_frame(0, bgcolor=[0, 0, 0])
    # image mode follows cfg.test.head_id (default -1), whatever the split
    heads_cfg.multihead = {'head_num': 3, 'split': 'view'}
    assert subject.movement_frame(0, image_size=(64, 64))['head_id'] == -1
    heads_cfg.test = {'head_id': 2}
    assert subject.movement_frame(0, image_size=(64, 64))['head_id'] == 2
    batch = dataset.to_device(subject.train_frame(1, bgcolor=[0, 0, 0]), 'cpu', host_keys=('patch_div_indices', 'head_id'))
    assert batch['head_id'].device.type == 'cpu' and int(batch['head_id']) == 0
    # a single-head configuration: items carry no head_id
    heads_cfg.canonical_mlp.multihead = {'enable': False}
    assert 'head_id' not in subject.train_frame(0, bgcolor=[0, 0, 0])
