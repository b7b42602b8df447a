"""The shared evaluation of underflowing inputs for all heads (include/hnrf_heads_shared.h) without a GPU: the four
entries and where they are bound, the workspace statement, the refusals that come back before a device is touched, and
the numpy twin of the n-plane fill (humannerf_amd.shared_input.fill_planes) on the K1 windows that
tests/test_shared_fused_cpu.py shows to hold both classes.  tests/test_gpu_heads_shared.py compares the kernels with
that twin."""
import ctypes

import numpy as np
import pytest

from humannerf_amd import shared_input as si
from tests import test_shared_fused_cpu as cases
from tests import test_shared_input_cpu as cpu
from tests.test_shared_fused_cpu import e2e_frame, representative  # noqa: F401  (fixtures)

F = np.float32
CANARY = F(7.0)
NAMES = ['hnrf_render_frame_heads_shared_fwd', 'hnrf_render_frame_heads_shared_workspace_bytes',
         'hnrf_sample_warp_share_heads_fwd', 'hnrf_share_compact_heads']
E_ARG, E_UNSUPPORTED = -1, -2


def head_c_raw(H):
    """c_raw (H, 4) with 4 H different values, none the canary, a -0 among them: a plane mix-up shows."""
    c = (np.arange(4 * H, dtype=F).reshape(H, 4) + F(1.0)) * F(0.25) * np.where(np.arange(4) % 2 == 0, F(1), F(-1))
    c[0, 3] = F(-0.0)
    assert np.unique(c.view(np.uint32)).size == 4 * H and not (c == CANARY).any()
    return c.astype(F)


# ------------------------------------------------------------------------------------- the entries and their table
def test_header_declares_the_four_entries():
    from humannerf_amd import _lib
    sigs = _lib.HEADS_SHARED_SIGNATURES
    assert sorted(sigs) == NAMES
    assert _lib.HEADS_SHARED_HEADER_PATH.replace('\\', '/').endswith('/include/hnrf_heads_shared.h')
    vp, i64, i, sz, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
    # hnrf_share_compact / hnrf_sample_warp_share_fwd with n_heads behind P / behind c_raw
    assert sigs['hnrf_share_compact_heads'] == (i, [vp] * 4 + [i64, i] + [vp] * 6)
    assert sigs['hnrf_share_compact_heads'][1] == (_lib.SIGNATURES['hnrf_share_compact'][1][:5] + [i]
                                                   + _lib.SIGNATURES['hnrf_share_compact'][1][5:])
    assert sigs['hnrf_sample_warp_share_heads_fwd'] == (i, [vp] * 10 + [i64, i, i, i] + [vp] * 7 + [i] + [vp] * 6)
    assert sigs['hnrf_sample_warp_share_heads_fwd'][1] == (_lib.SIGNATURES['hnrf_sample_warp_share_fwd'][1][:21] + [i]
                                                           + _lib.SIGNATURES['hnrf_sample_warp_share_fwd'][1][21:])
    assert sigs['hnrf_render_frame_heads_shared_workspace_bytes'] == (sz, [i64, i, i])
    # hnrf_render_frame_heads_fwd plus live_counts behind offsets
    heads = _lib.HEADS_SIGNATURES['hnrf_render_frame_heads_fwd'][1]
    assert sigs['hnrf_render_frame_heads_shared_fwd'] == (i, [vp] * 14 + [i, f, i64, i, i, i, i64, i, vp, sz] + [vp] * 16)
    assert sigs['hnrf_render_frame_heads_shared_fwd'][1] == heads[:35] + [vp] + heads[35:]
    others = [_lib.SIGNATURES, _lib.CLOUD_SIGNATURES, _lib.VIDEO_SIGNATURES, _lib.SEGMENT_SIGNATURES,
              _lib.GEOMETRY_SIGNATURES, _lib.HEADS_SIGNATURES, _lib.SKIN_SIGNATURES]
    for table in others:
        assert not set(sigs) & set(table)


def test_open_table_and_versions(monkeypatch):
    import subprocess

    import __graft_entry__ as entry
    from humannerf_amd import _lib
    assert 'heads_shared' in _lib.OPEN_GROUPS
    assert 'heads_shared' not in _lib.GROUPS and 'heads_shared' not in _lib.LATE_GROUPS
    assert _lib.OPEN_GROUPS['heads_shared'][0] == 'hnrf_heads_shared.h'
    lib = _lib.load_heads_shared()
    assert lib is _lib.load() and _lib.load_open() is lib
    assert lib.hnrf_abi_version() == 13 and len(_lib.SIGNATURES) == 88
    assert sorted(_lib.HEADS_SIGNATURES) == ['hnrf_canonical_heads_fwd', 'hnrf_canonical_heads_fwd_sparse',
                                             'hnrf_canonical_heads_pack', 'hnrf_render_frame_heads_fwd',
                                             'hnrf_render_frame_heads_workspace_bytes']
    for name in NAMES:
        assert hasattr(lib, name)
        assert (getattr(lib, name).restype, getattr(lib, name).argtypes) == _lib.HEADS_SHARED_SIGNATURES[name]
    # a library from before the header: the rebuild message, from load_heads_shared alone
    with pytest.raises(_lib.HnrfError, match=r'built before the shared evaluation for all heads \(include/hnrf_heads_shared.h\)'):
        _lib.load_heads_shared(type('OldLib', (), {})())
    # build() binds the open table, through _bind_table
    seen = []
    real = _lib._bind_table
    monkeypatch.setattr(_lib, '_bind_table', lambda group, lib, table, headers: seen.append((group, table)) or
                        real(group, lib, table, headers))
    monkeypatch.setattr(subprocess, 'run', lambda *a, **kw: None)          # (the library is built: no make)
    entry.build()
    assert ('heads_shared', _lib.OPEN_GROUPS) in seen


@pytest.mark.parametrize('H', [2, 3, 8])
def test_workspace_holds_the_slot_and_a_second_plane_set(H):
    from humannerf_amd import _lib
    lib = _lib.load_heads_shared()
    _lib.load_heads()
    need = lib.hnrf_render_frame_heads_shared_workspace_bytes(96, 16, H)
    assert need >= lib.hnrf_render_frame_heads_workspace_bytes(96, 16, H) + 256 + H * 96 * 16 * 16
    assert need % 256 == 0
    # the slot sits where hnrf_render_frame_shared_fwd has it, and 4 H floats of c_raw fit behind float 12
    assert 4 * (12 + 4 * H) <= 256


def test_workspace_is_zero_outside_2_to_8_heads():
    from humannerf_amd import _lib
    lib = _lib.load_heads_shared()
    for H in (1, 9):
        assert lib.hnrf_render_frame_heads_shared_workspace_bytes(96, 16, H) == 0
    assert lib.hnrf_render_frame_heads_shared_workspace_bytes(-1, 16, 3) == 0


def test_argument_errors_before_a_device_is_touched():
    from humannerf_amd import _lib
    lib = _lib.load_heads_shared()
    err = lambda: lib.hnrf_last_error().decode()
    buf = (ctypes.c_int * 16)()
    some = ctypes.addressof(buf)                                     # (a non-null pointer nobody follows)
    # hnrf_share_compact_heads
    assert lib.hnrf_share_compact_heads(*[None] * 4, 4, 3, *[None] * 6) == E_ARG and 'null pointer' in err()
    assert lib.hnrf_share_compact_heads(*[some] * 4, 4, 9, *[some] * 5, None) == E_ARG and 'n_heads=9' in err()
    assert lib.hnrf_share_compact_heads(*[some] * 4, 4, 1, *[some] * 5, None) == E_ARG and 'n_heads=1' in err()
    assert lib.hnrf_share_compact_heads(*[some] * 4, -1, 3, *[some] * 5, None) == E_ARG and 'bad P' in err()
    assert lib.hnrf_share_compact_heads(*[some] * 4, 4, 3, some, some, some, None, some, None) == E_ARG
    assert 'offsets and xyz' in err()
    assert lib.hnrf_share_compact_heads(*[some] * 4, 4, 3, *[some] * 4, some + 4, None) == E_ARG and 'aligned' in err()
    # hnrf_sample_warp_share_heads_fwd
    k1 = lambda B, H, p: lib.hnrf_sample_warp_share_heads_fwd(*[p] * 10, 2, 16, B, 32, *[p] * 7, H, *[p] * 5, None)
    assert k1(24, 3, None) == E_ARG and 'null pointer' in err()
    assert k1(24, 9, some) == E_ARG and 'n_heads=9' in err()
    assert k1(24, 0, some) == E_ARG and 'n_heads=0' in err()
    assert k1(23, 3, some) == E_UNSUPPORTED and '24 bones' in err() and 'hnrf_sample_warp_share_heads_fwd' in err()
    # hnrf_render_frame_heads_shared_fwd
    frame = lambda H, live, planes: lib.hnrf_render_frame_heads_shared_fwd(
        *[some] * 14, 1, 0.0, 8, 16, 24, 32, 8, H, some, 1 << 30, *[planes] * 3, *[None] * 8, live, None, None, None, None)
    assert frame(3, None, some) == E_ARG and 'live_counts' in err()
    assert frame(9, some, some) == E_ARG and 'n_heads=9' in err()
    assert frame(1, some, some) == E_ARG and 'n_heads=1' in err()
    assert frame(3, some, None) == E_ARG and 'null output array' in err()
    planes = (ctypes.c_void_p * 3)(some, some, None)
    assert frame(3, some, planes) == E_ARG and 'plane of head 2' in err()


# ------------------------------------------------------------------------------------- the twin
def test_twin_on_the_crafted_problem():
    """Every value class of the predicate: plane g of the n-plane fill is the single-plane fill with c_raw[g]."""
    x, cs = cpu.crafted_problem()
    P = x.shape[0]
    for H in (1, 2, 8):
        c_raw = head_c_raw(H)
        for c, cx in cs:
            planes = np.full((H, P, 4), CANARY, dtype=F)
            live = si.fill_planes(x, c, cx, c_raw, planes)
            m = si.shared_mask(x, c, cx)
            assert np.array_equal(live, si.live_indices(x, c, cx)) and live.size == int((~m).sum())
            for g in range(H):
                assert np.array_equal(planes[g, m].view(np.uint32), np.broadcast_to(c_raw[g].view(np.uint32), (int(m.sum()), 4)))
                assert (planes[g, ~m] == CANARY).all()
    with pytest.raises(ValueError):
        si.fill_planes(x, cs[0][0], cs[0][1], head_c_raw(3), np.zeros((2, P, 4), F))


@pytest.mark.parametrize('H', [2, 8])
@pytest.mark.parametrize('case', sorted(k for k, v in cases.CASES.items() if v[3]))
def test_twin_on_the_k1_windows(seeded_params, e2e_frame, representative, case, H):  # noqa: F811
    """The windows of tests/test_shared_fused_cpu.py that hold both classes, x_skel from the fp32 oracle: every shared
    row of plane g holds head g's constants, every live row of every plane keeps the canary, and the live list is the
    single-head one."""
    from oracle import oracle
    r0, R, S, both = cases.CASES[case]
    assert both
    c, cx, x_frame = representative
    if case == 'frame':
        x = x_frame
    else:
        x = oracle.render(seeded_params, cases.window(e2e_frame, r0, R), iter_val=1e7,
                          N_samples=S)['_x_skel'].numpy().reshape(-1, 3)
    P = R * S
    c_raw = head_c_raw(H)
    planes = np.full((H, P, 4), CANARY, dtype=F)
    live = si.fill_planes(x, c, cx, c_raw, planes)
    assert np.array_equal(live, si.live_indices(x, c, cx)) and 0 < live.size < P
    shared = np.ones(P, dtype=bool)
    shared[live] = False
    for g in range(H):
        assert (planes[g, live] == CANARY).all()
        assert not (planes[g, shared] == CANARY).any()
        assert np.array_equal(planes[g, shared].view(np.uint32),
                              np.broadcast_to(c_raw[g].view(np.uint32), (int(shared.sum()), 4)))
    assert not np.array_equal(planes[0], planes[1])
