"""The shared evaluation of underflowing inputs for all heads on the GPU (include/hnrf_heads_shared.h): the n-plane
classification, fused into K1 and stand-alone, against each other and against the numpy twin
(humannerf_amd.shared_input.fill_planes); the frame entry against hnrf_render_frame_heads_fwd; and
Network.forward(head_id=-1) with cfg.amd.share_underflow on against off and against forward(head_id=h).  The feature
promises the same bits, so every comparison is torch.equal on the integer view.  tests/test_heads_shared_cpu.py holds
the twin's own checks."""
import ctypes

import numpy as np
import pytest
import torch

import multihead_cases as mc
from humannerf_amd import shared_input as si
from tests import test_shared_fused_cpu as cases
from tests import test_shared_input_cpu as cpu
from tests.test_gpu_shared_fused import CANARY, _both_ways, _canaries, _k1_args, _ptr, k1_inputs  # noqa: F401
from tests.test_gpu_shared_input import (AMD_KEYS, KEYS11, G, _stream, bits, dev, frame, net, nr_problem,  # noqa: F401
                                         options)
from tests.test_heads_shared_cpu import head_c_raw

pytestmark = pytest.mark.gpu

F = np.float32
PER_HEAD = KEYS11[:8]
CHUNK = 100                                   # 576 rays: five whole chunks and one of 76


# ------------------------------------------------------------------------------------- 1. fused vs unfused vs twin
def _heads_both_ways(args, R, S, c_off, c_xyz, c_raw, H, lean, want_bmw):
    """(unfused, fused): hnrf_sample_warp_fwd + hnrf_share_compact_heads, and hnrf_sample_warp_share_heads_fwd, into
    canaries; raw is (H, P, 4)."""
    from humannerf_amd import _lib
    lib = _lib.load_heads_shared()
    B, Gv = args[5].shape[0], args[7].shape[-1]
    P = R * S
    a, b = _canaries(P, B, lean, want_bmw), _canaries(P, B, lean, want_bmw)
    for o in (a, b):
        o['raw'] = torch.full((H, P, 4), CANARY, device=dev())
    ptrs = [_ptr(t) for t in args]
    _lib.check(lib.hnrf_sample_warp_fwd(*ptrs, R, S, B, Gv, _ptr(a['z']), _ptr(a['x_skel']), _ptr(a['mask']), _ptr(a['bmw']),
                                        _stream()), 'hnrf_sample_warp_fwd')
    _lib.check(lib.hnrf_share_compact_heads(_ptr(a['x_skel']), _ptr(c_off), _ptr(c_xyz), _ptr(c_raw), P, H, _ptr(a['idx']),
                                            _ptr(a['count']), _ptr(a['offsets']), _ptr(a['xyz']), _ptr(a['raw']), _stream()),
               'hnrf_share_compact_heads')
    _lib.check(lib.hnrf_sample_warp_share_heads_fwd(*ptrs, R, S, B, Gv, _ptr(b['z']), _ptr(b['x_skel']), _ptr(b['mask']),
                                                    _ptr(b['bmw']), _ptr(c_off), _ptr(c_xyz), _ptr(c_raw), H, _ptr(b['idx']),
                                                    _ptr(b['count']), _ptr(b['offsets']), _ptr(b['xyz']), _ptr(b['raw']),
                                                    _stream()), 'hnrf_sample_warp_share_heads_fwd')
    torch.cuda.synchronize()
    return a, b


def _check_heads(a, b, c_off, c_xyz, c_raw, H, lean, want_bmw):
    """The fused and the unfused form agree bit for bit, and both are the twin.  Returns (count, P, sorted live list)."""
    P = a['z'].numel()
    for k in ('z', 'x_skel', 'mask') + (('bmw',) if want_bmw else ()):
        assert torch.equal(bits(a[k]), bits(b[k])), k
        assert not bool((b[k] == CANARY).all()), k
    x = b['x_skel'].cpu().numpy()
    twin = np.full((H, P, 4), CANARY, dtype=F)
    live = si.fill_planes(x, c_off.cpu().numpy(), c_xyz.cpu().numpy(), c_raw.cpu().numpy(), twin)
    count = int(b['count'].item())
    assert count == int(a['count'].item()) == live.size                # each live sample once, whatever H is
    for o in (a, b):
        idx = o['idx'].cpu().numpy()
        assert np.array_equal(np.sort(idx[:count]), live)              # (block order on the device: the same set)
        assert (idx[count:] == -1).all()
        # live rows keep the canary in every plane, shared rows hold head g's constants in plane g
        assert torch.equal(bits(o['raw']), bits(G(twin)))
    m = torch.ones(P, dtype=torch.bool, device=dev())
    m[torch.from_numpy(live.astype(np.int64)).to(dev())] = False       # the shared rows
    for k, want in (('offsets', c_off), ('xyz', c_xyz)):
        if lean:
            assert a[k] is None and b[k] is None
            continue
        assert torch.equal(bits(a[k]), bits(b[k])), k
        assert bool((b[k][~m] == CANARY).all()), k
        assert torch.equal(bits(b[k][m]), bits(want)[None].expand(int(m.sum()), 3)), k
    return count, P, live


@pytest.mark.parametrize('lean', [False, True], ids=['diag', 'lean'])
@pytest.mark.parametrize('H', [2, 8])
@pytest.mark.parametrize('case', sorted(cases.CASES))
def test_fused_equals_unfused_equals_twin(k1_inputs, nr_problem, case, H, lean):  # noqa: F811
    r0, R, S, both = cases.CASES[case]
    s = nr_problem
    c_raw = G(head_c_raw(H))
    args = _k1_args(*k1_inputs, r0, R)
    want_bmw = not lean                                                # (both K1 instances with the n-plane form)
    a, b = _heads_both_ways(args, R, S, s['c_off'], s['c_xyz'], c_raw, H, lean, want_bmw)
    count, P, live = _check_heads(a, b, s['c_off'], s['c_xyz'], c_raw, H, lean, want_bmw)
    print('%s H=%d: P = %d, live %d' % (case, H, P, count))
    assert P == R * S
    if both:
        assert 0 < count < P
        assert not torch.equal(b['raw'][0], b['raw'][1])               # the planes hold different constants
    # idx[0 .. count) and count are the single-head entry's
    one, _ = _both_ways(args, R, S, s['c_off'], s['c_xyz'], c_raw[0].contiguous(), lean, want_bmw)
    assert int(one['count'].item()) == count
    assert np.array_equal(np.sort(one['idx'].cpu().numpy()[:count]), live)
    assert torch.equal(bits(one['raw']), bits(b['raw'][0]))            # and plane 0 is its raw


@pytest.mark.parametrize('H', [2, 8])
def test_all_shared_and_none_shared_windows(k1_inputs, nr_problem, H):  # noqa: F811
    """An all-zero weight volume: x_skel is exactly 0, count == 0 and every plane is fully written.  A c_xyz that is
    not 0 + c_off: condition (b) fails everywhere, every sample is listed and every plane is untouched."""
    fr, Rs, Ts, vol = k1_inputs
    r0, R, S, _ = cases.CASES['P3073']
    s = nr_problem
    c_raw = G(head_c_raw(H))
    a, b = _heads_both_ways(_k1_args(fr, Rs, Ts, torch.zeros_like(vol), r0, R), R, S, s['c_off'], s['c_xyz'], c_raw, H,
                            False, True)
    count, P, _ = _check_heads(a, b, s['c_off'], s['c_xyz'], c_raw, H, False, True)
    assert count == 0 and bool((b['x_skel'] == 0).all())
    assert torch.equal(bits(b['raw']), bits(c_raw)[:, None, :].expand(H, P, 4))
    c_xyz = s['c_xyz'] + 1.0
    a, b = _heads_both_ways(_k1_args(fr, Rs, Ts, vol, r0, R), R, S, s['c_off'], c_xyz, c_raw, H, True, False)
    count, P, _ = _check_heads(a, b, s['c_off'], c_xyz, c_raw, H, True, False)
    assert count == P
    assert bool((a['raw'] == CANARY).all()) and bool((b['raw'] == CANARY).all())


def test_fused_heads_k1_wants_24_bones(k1_inputs, nr_problem):  # noqa: F811
    from humannerf_amd import _lib
    fr, Rs, Ts, vol = k1_inputs
    args = _k1_args(fr, Rs[:23].contiguous(), Ts[:23].contiguous(), vol, 0, 2)
    with pytest.raises(_lib.HnrfError, match='24 bones'):
        _heads_both_ways(args, 2, 128, nr_problem['c_off'], nr_problem['c_xyz'], G(head_c_raw(2)), 2, True, False)


# ------------------------------------------------------------------------------------- 2. the frame through Network
H_NET = 3


@pytest.fixture(scope='module')
def heads_net(seeded_params):
    """A Network with H_NET heads on the seeded multi-head state; the configuration is restored at once."""
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network
    keep = (cfg.get('multihead'), cfg.canonical_mlp.get('multihead'))
    cfg.canonical_mlp.multihead = {'enable': True, 'head_depth': 1}
    cfg.multihead = {'head_num': H_NET, 'split': 'view'}
    try:
        n = Network()
    finally:
        for node, key, val in ((cfg, 'multihead', keep[0]), (cfg.canonical_mlp, 'multihead', keep[1])):
            if val is None:
                node.pop(key)
            else:
                node[key] = val
    state = mc.multihead_state(seeded_params, H_NET)
    n.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()}, strict=True)
    return n.to(dev()).eval()


def _render_head(n, fr, cfg, share, head_id):
    """One frame from a fresh guard schedule: (outputs, share of shared samples); the f16-range verdict is clean."""
    cfg.amd.share_underflow = share
    n.f16_guard.restart_schedule()
    with torch.no_grad():
        out = n(**fr, iter_val=1e7, head_id=head_id)
    s = n.shared_sample_share()
    assert n.check_f16_range(wait=True) is False
    return out, s


def _frame_options(cfg, diag, overlap, mode='f16x3'):
    cfg.chunk = CHUNK
    cfg.amd.diagnostics = diag
    cfg.amd.f16_range_guard = 'audit'
    cfg.amd.overlap_warp = overlap
    cfg.amd.mlp_mode = mode


def _same_heads_frame(on, off, diag):
    assert set(on) == set(off) == set(KEYS11 if diag else KEYS11[:3])
    for k in on:
        if isinstance(off[k], list):
            assert isinstance(on[k], list) and len(on[k]) == len(off[k]) == H_NET
            for h in range(H_NET):
                assert torch.equal(bits(on[k][h]), bits(off[k][h])), (k, h)
        else:
            assert torch.equal(bits(on[k]), bits(off[k])), k


@pytest.mark.parametrize('overlap', [False, True], ids=['one_stream', 'overlap'])
@pytest.mark.parametrize('diag', [True, False], ids=['diag', 'lean'])
def test_all_heads_frame_on_equals_off(heads_net, frame, options, diag, overlap):  # noqa: F811
    """forward(head_id=-1) on the 24 x 24 frame at S = 128 in chunks of 100 rays -- six chunks, so both plane sets are
    used three times, with K1 on the side stream or not: every output with cfg.amd.share_underflow equals the output
    without it, head h of it equals forward(head_id=h), and the share of shared samples is the single-head frame's.
    (Before the all-heads path shared, shared_sample_share() was 0.0 after such a frame: this test failed.)"""
    cfg = options
    _frame_options(cfg, diag, overlap)
    n = heads_net
    off, s_off = _render_head(n, frame, cfg, False, -1)
    on, s_on = _render_head(n, frame, cfg, True, -1)
    assert n._share_last is not None and n._share_last[0].numel() == 6
    print('all heads, %s/%s: shared share %.6f' % ('diag' if diag else 'lean', overlap, s_on))
    assert s_off == 0.0
    _same_heads_frame(on, off, diag)
    keys = [k for k in PER_HEAD if diag or k in KEYS11[:3]]
    s_one = None
    for h in range(H_NET):
        one, s = _render_head(n, frame, cfg, True, h)
        s_one = s if h == 0 else s_one
        for k in keys:
            assert torch.equal(bits(on[k][h]), bits(one[k])), (k, h)
        if diag:
            assert torch.equal(bits(on['xyz_on_rays'][h]), bits(one['xyz_on_rays']))
            assert torch.equal(bits(on['offsets']), bits(one['offsets']))
            assert torch.equal(bits(on['backward_motion_weights']), bits(one['backward_motion_weights']))
    assert s_on == s_one                                            # the predicate does not depend on the head
    assert 0.05 < s_on < 0.95
    assert not torch.equal(on['rgb'][0], on['rgb'][1])              # the heads are different networks


@pytest.mark.parametrize('why', ['f32', 'cull'])
def test_all_heads_frame_takes_the_unshared_path(heads_net, frame, options, why):  # noqa: F811
    """Mode f32, or the option on with cfg.amd.cull_eps > 0 (lean form): the all-heads frame silently renders without
    the shared evaluation, as the single-head frame does, and equals the frame with the option off."""
    from humannerf_amd.config import amd_option
    cfg = options
    keep = amd_option('cull_eps', 0.0)
    _frame_options(cfg, False, True, 'f32' if why == 'f32' else 'f16x3')
    try:
        cfg.amd.cull_eps = 1e-3 if why == 'cull' else 0.0
        off, s_off = _render_head(heads_net, frame, cfg, False, -1)
        on, s_on = _render_head(heads_net, frame, cfg, True, -1)
    finally:
        cfg.amd.cull_eps = keep
    assert s_off == 0.0 and s_on == 0.0 and heads_net._share_last is None
    _same_heads_frame(on, off, False)


# ------------------------------------------------------------------------------------- 3. the entry, called directly
def _heads_image(seeded_params, H):
    from humannerf_amd import ops
    st = mc.multihead_state(seeded_params, H)
    names = ['cnl_mlp.module.pts_linears.%d' % i for i in range(0, 16, 2)] + ['cnl_mlp.module.output_linear.0']
    return ops.canonical_heads_pack([G(st[k + '.weight']) for k in names], [G(st[k + '.bias']) for k in names], H, 'f16x3')


@pytest.mark.parametrize('H', [2, 8])
def test_frame_entry_direct_abi(seeded_params, k1_inputs, nr_problem, H):  # noqa: F811
    """hnrf_render_frame_heads_shared_fwd through ctypes with a workspace of exactly the stated size: every plane and
    every single buffer equals hnrf_render_frame_heads_fwd's, with and without the diagnostic outputs; the live counts
    add up to the twin's on the frame's x_skel; the slot holds c_raw [H][4]; and the refusals leave the outputs alone."""
    from humannerf_amd import _lib, ops
    lib = _lib.load_heads_shared()
    _lib.load_heads()
    fr, Rs, Ts, vol = k1_inputs
    s = nr_problem
    N, S, B, Gv = 576, cpu.E2E_SAMPLES, Rs.shape[0], vol.shape[-1]
    k1 = _k1_args(fr, Rs, Ts, vol, 0, N)
    packed = _heads_image(seeded_params, H)
    bg = G(np.asarray(fr['bgcolor'], dtype=F))
    args = [_ptr(t) for t in k1 + [s['hann'], s['packed'], packed, bg]]
    mode = ops._mode_arg('f16x3')
    need = lib.hnrf_render_frame_heads_shared_workspace_bytes(CHUNK, S, H)
    need_off = lib.hnrf_render_frame_heads_workspace_bytes(CHUNK, S, H)
    assert need % 4 == 0 and need >= need_off + 256 + H * CHUNK * S * 16
    ws, ws_off = torch.empty(need // 4, device=dev()), torch.empty(need_off // 4, device=dev())
    nchunk = -(-N // CHUNK)
    # the twin's live count: K1 on the whole frame, the representative of this non-rigid image
    a, _ = _both_ways(k1, N, S, s['c_off'], s['c_xyz'], torch.zeros(4, device=dev()), True, False)
    want_live = si.live_indices(a['x_skel'].cpu().numpy(), s['c_off'].cpu().numpy(), s['c_xyz'].cpu().numpy()).size
    assert 0 < want_live < N * S

    def buffers(diag):
        shapes = ops.output_shapes(S, B, diag)
        planes = {k: torch.full((H, N) + shapes[k], -7.0, device=dev()) for k in PER_HEAD if k in shapes}
        single = {k: torch.full((N,) + v, -7.0, device=dev()) for k, v in shapes.items() if k not in PER_HEAD}
        arr = [(ctypes.c_void_p * H)(*[planes[k][h].data_ptr() for h in range(H)]) if k in planes else None for k in PER_HEAD]
        tail = [_ptr(single.get(k)) for k in ('xyz_on_rays', 'backward_motion_weights', 'offsets')]
        return planes, single, arr + tail

    def untouched(planes, single):
        torch.cuda.synchronize()
        return all(bool((t == -7.0).all()) for t in list(planes.values()) + list(single.values()))

    for diag in (True, False):
        p_off, s_off, out_off = buffers(diag)
        rc = lib.hnrf_render_frame_heads_fwd(*args, mode, 0.0, N, S, B, Gv, CHUNK, H, ws_off.data_ptr(), need_off, *out_off,
                                             None, None, None, _stream())
        assert rc == 0, lib.hnrf_last_error()
        p_on, s_on, out_on = buffers(diag)
        live = torch.full((nchunk,), -1, dtype=torch.int32, device=dev())
        head = (*args, mode, 0.0, N, S, B, Gv, CHUNK, H)
        rc = lib.hnrf_render_frame_heads_shared_fwd(*head, ws.data_ptr(), need, *out_on, live.data_ptr(), None, None, None,
                                                    _stream())
        assert rc == 0, lib.hnrf_last_error()
        torch.cuda.synchronize()
        for k in p_off:
            assert torch.equal(bits(p_on[k]), bits(p_off[k])), (diag, k)
            assert not bool((p_on[k] == -7.0).all()), k
        for k in s_off:
            assert torch.equal(bits(s_on[k]), bits(s_off[k])), (diag, k)
        assert set(s_off) == ({'xyz_on_rays', 'backward_motion_weights', 'offsets'} if diag else set())
        assert not torch.equal(p_on['rgb'][0], p_on['rgb'][1])
        assert bool((live >= 0).all()) and int(live.sum().item()) == want_live
        # the representative slot behind the two chunk workspaces: x = 0 | c_off | c_xyz | c_raw [H][4]
        at = 2 * lib.hnrf_render_workspace_bytes(CHUNK, S) // 4
        slot = ws[at:at + 64].clone()
        assert bool((slot[:4] == 0).all())
        assert torch.equal(bits(slot[4:7]), bits(s['c_off'])) and torch.equal(bits(slot[8:11]), bits(s['c_xyz']))
        c_raw = ops.canonical_heads(s['c_xyz'][None].contiguous(), packed, H, 'f16x3')
        assert torch.equal(bits(slot[12:12 + 4 * H]), bits(c_raw.reshape(-1)))
        # refused before anything runs: the outputs keep their canary
        planes, single, out = buffers(diag)
        tail = (None, None, None, _stream())
        assert lib.hnrf_render_frame_heads_shared_fwd(*head, ws.data_ptr(), need - 1, *out, live.data_ptr(), *tail) == -4
        assert lib.hnrf_render_frame_heads_shared_fwd(*head, ws.data_ptr(), need, *out, None, *tail) == -1
        assert b'live_counts' in lib.hnrf_last_error()
        culled = (*args, mode, 1e-3, N, S, B, Gv, CHUNK, H)
        assert lib.hnrf_render_frame_heads_shared_fwd(*culled, ws.data_ptr(), need, *out, live.data_ptr(), *tail) != 0
        f32 = (*args, ops._mode_arg('f32'), 0.0, N, S, B, Gv, CHUNK, H)
        assert lib.hnrf_render_frame_heads_shared_fwd(*f32, ws.data_ptr(), need, *out, live.data_ptr(), *tail) == -2
        assert b'HNRF_MLP_F16X3' in lib.hnrf_last_error()
        assert untouched(planes, single)
