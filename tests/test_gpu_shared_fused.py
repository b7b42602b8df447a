"""The fused form of cfg.amd.share_underflow (include/hnrf.h, hnrf_sample_warp_share_fwd): K1 classifies the samples it
has just warped, lists the live ones and fills the shared rows.  Everything here is a statement about bits -- the fused
K1 against K1 + hnrf_share_compact, the frame against the frame without the option -- so every comparison is
torch.equal on the integer view.  tests/test_shared_fused_cpu.py chooses the K1 cases and shows on the CPU that they
hold both classes.  (The gathered K2 / K3 forms the same work tried -- inputs compacted next to the list -- gained
nothing and are not in the library: profiles/shared_fused.txt.)"""
import numpy as np
import pytest
import torch

from humannerf_amd import shared_input as si
from tests import test_shared_fused_cpu as cases
from tests import test_shared_input_cpu as cpu
from tests.test_gpu_shared_input import (AMD_KEYS, KEYS11, G, _assert_same, _net, _render, _stream, bits, dev,  # noqa: F401
                                         frame, net, nr_problem, options)

pytestmark = pytest.mark.gpu

F = np.float32
CANARY = 7.0
CNL = 'cnl_mlp.module.pts_linears.'


# ------------------------------------------------------------------------------------- 1. fused K1 vs K1 + share_compact
@pytest.fixture(scope='module')
def k1_inputs(net):
    """K1's inputs for the end-to-end frame as Network.forward prepares them (numpy frame, device motion basis)."""
    from humannerf_amd import scene
    fr = scene.synthetic_frame(**cpu.E2E_FRAME)
    Rs, Ts, vol = net.frame_motion(fr)
    return fr, Rs.contiguous(), Ts.contiguous(), vol.contiguous()


def _k1_args(fr, Rs, Ts, vol, r0, R):
    w = cases.window(fr, r0, R)
    return [G(w['rays'][0]), G(w['rays'][1]), G(w['near'].reshape(-1)), G(w['far'].reshape(-1)), None, Rs, Ts, vol,
            G(fr['cnl_bbox_min_xyz']), G(fr['cnl_bbox_scale_xyz'])]


def _canaries(P, B, lean, want_bmw):
    t = lambda *s: torch.full(s, CANARY, device=dev())
    o = dict(z=t(P), x_skel=t(P, 3), mask=t(P), raw=t(P, 4),
             idx=torch.full((P,), -1, dtype=torch.int32, device=dev()),
             count=torch.full((1,), 12345, dtype=torch.int32, device=dev()))          # (the entries zero it)
    o['bmw'] = t(P, B) if want_bmw else None
    o['offsets'], o['xyz'] = (None, None) if lean else (t(P, 3), t(P, 3))
    return o


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _both_ways(args, R, S, c_off, c_xyz, c_raw, lean, want_bmw):
    """(unfused, fused): hnrf_sample_warp_fwd + hnrf_share_compact, and hnrf_sample_warp_share_fwd, into canaries."""
    from humannerf_amd import _lib
    lib = _lib.load()
    B, Gv = args[5].shape[0], args[7].shape[-1]
    P = R * S
    a, b = _canaries(P, B, lean, want_bmw), _canaries(P, B, lean, want_bmw)
    ptrs = [_ptr(t) for t in args]
    _lib.check(lib.hnrf_sample_warp_fwd(*ptrs, R, S, B, Gv, _ptr(a['z']), _ptr(a['x_skel']), _ptr(a['mask']), _ptr(a['bmw']),
                                        _stream()), 'hnrf_sample_warp_fwd')
    _lib.check(lib.hnrf_share_compact(_ptr(a['x_skel']), _ptr(c_off), _ptr(c_xyz), _ptr(c_raw), P, _ptr(a['idx']),
                                      _ptr(a['count']), _ptr(a['offsets']), _ptr(a['xyz']), _ptr(a['raw']), _stream()),
               'hnrf_share_compact')
    _lib.check(lib.hnrf_sample_warp_share_fwd(*ptrs, R, S, B, Gv, _ptr(b['z']), _ptr(b['x_skel']), _ptr(b['mask']),
                                              _ptr(b['bmw']), _ptr(c_off), _ptr(c_xyz), _ptr(c_raw), _ptr(b['idx']),
                                              _ptr(b['count']), _ptr(b['offsets']), _ptr(b['xyz']), _ptr(b['raw']), _stream()),
               'hnrf_sample_warp_share_fwd')
    torch.cuda.synchronize()
    return a, b


def _check_fused(a, b, c_off, c_xyz, lean, want_bmw):
    """Every statement of the issue's test 1; returns (count, P)."""
    P = a['z'].numel()
    for k in ('z', 'x_skel', 'mask') + (('bmw',) if want_bmw else ()):
        assert torch.equal(bits(a[k]), bits(b[k])), k
        assert not bool((b[k] == CANARY).all()), k
    count = int(b['count'].item())
    assert count == int(a['count'].item())
    x = b['x_skel'].cpu().numpy()
    live = si.live_indices(x, c_off.cpu().numpy(), c_xyz.cpu().numpy())
    assert count == live.size
    idx = b['idx'].cpu().numpy()
    assert np.array_equal(np.sort(idx[:count]), live)
    assert np.array_equal(np.sort(a['idx'].cpu().numpy()[:count]), live)
    assert (idx[count:] == -1).all()
    il = torch.from_numpy(idx[:count].astype(np.int64)).to(dev())
    m = torch.ones(P, dtype=torch.bool, device=dev())
    m[il] = False                                                    # the shared rows
    for k in ('raw', 'offsets', 'xyz'):
        if lean and k != 'raw':
            assert a[k] is None and b[k] is None
            continue
        assert torch.equal(bits(a[k]), bits(b[k])), k                # fills on the shared rows, canaries on the live ones
        assert bool((b[k][~m] == CANARY).all()), k
        assert not bool((b[k][m] == CANARY).any()), k
    return count, P


@pytest.mark.parametrize('lean', [False, True], ids=['diag', 'lean'])
@pytest.mark.parametrize('want_bmw', [True, False], ids=['bmw', 'nobmw'])
@pytest.mark.parametrize('case', sorted(cases.CASES))
def test_fused_k1_equals_k1_then_share_compact(k1_inputs, nr_problem, case, want_bmw, lean):
    r0, R, S, both = cases.CASES[case]
    c_raw = G(np.array([0.25, -1.5, 3.0, -0.0], dtype=F))
    a, b = _both_ways(_k1_args(*k1_inputs, r0, R), R, S, nr_problem['c_off'], nr_problem['c_xyz'], c_raw, lean, want_bmw)
    count, P = _check_fused(a, b, nr_problem['c_off'], nr_problem['c_xyz'], lean, want_bmw)
    print('%s: P = %d, live %d' % (case, P, count))
    assert P == R * S
    if both:
        assert 0 < count < P
    if case == 'frame':
        assert abs((1.0 - count / P) - 0.42) < 0.02


@pytest.mark.parametrize('lean', [False, True], ids=['diag', 'lean'])
def test_fused_k1_all_shared_then_noop_mlps(k1_inputs, nr_problem, lean):
    """An all-zero weight volume: x_skel is exactly 0, everything is shared, count == 0, and K2 / K3 launched on that
    empty list, as the frame launches them, write nothing."""
    from humannerf_amd import _lib, ops
    fr, Rs, Ts, vol = k1_inputs
    r0, R, S, _ = cases.CASES['P3073']
    s = nr_problem
    c_raw = G(np.array([0.25, -1.5, 3.0, -0.0], dtype=F))
    a, b = _both_ways(_k1_args(fr, Rs, Ts, torch.zeros_like(vol), r0, R), R, S, s['c_off'], s['c_xyz'], c_raw, lean, True)
    count, P = _check_fused(a, b, s['c_off'], s['c_xyz'], lean, True)
    assert count == 0 and bool((b['x_skel'] == 0).all())
    if lean:
        b['xyz'] = torch.full((P, 3), CANARY, device=dev())          # (the lean form's xyz lives in the workspace)
    keep = {k: v.clone() for k, v in b.items() if v is not None}
    lib = _lib.load()
    cp = _cnl_packed_of(None)
    xyz = b['xyz']
    for mode in ('f16x3', 'f16x3+noguard'):
        _lib.check(lib.hnrf_nonrigid_fwd_sparse(_ptr(b['x_skel']), _ptr(s['hann']), _ptr(s['packed']), ops._mode_arg(mode), P,
                                                _ptr(b['idx']), _ptr(b['count']), _ptr(xyz), _ptr(b['offsets']), _stream()),
                   'hnrf_nonrigid_fwd_sparse')
        _lib.check(lib.hnrf_canonical_fwd_sparse(_ptr(xyz), _ptr(cp), ops._mode_arg(mode), P, _ptr(b['idx']), _ptr(b['count']),
                                                 _ptr(b['raw']), _stream()), 'hnrf_canonical_fwd_sparse')
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(bits(v) if v.dtype == torch.float32 else v, bits(b[k]) if v.dtype == torch.float32 else b[k]), k


@pytest.mark.parametrize('lean', [False, True], ids=['diag', 'lean'])
def test_fused_k1_no_shared_sample(k1_inputs, nr_problem, lean):
    """No sample is shared -- condition (b) fails everywhere: c_xyz is not 0 + c_off --: every sample is listed, no row
    is filled."""
    r0, R, S, _ = cases.CASES['P3073']
    s = nr_problem
    c_raw = G(np.array([0.25, -1.5, 3.0, -0.0], dtype=F))
    c_xyz = s['c_xyz'] + 1.0
    a, b = _both_ways(_k1_args(*k1_inputs, r0, R), R, S, s['c_off'], c_xyz, c_raw, lean, False)
    count, P = _check_fused(a, b, s['c_off'], c_xyz, lean, False)
    assert count == P
    assert bool((b['raw'] == CANARY).all())


def test_fused_k1_wants_24_bones(k1_inputs, nr_problem):
    from humannerf_amd import _lib
    fr, Rs, Ts, vol = k1_inputs
    args = _k1_args(fr, Rs[:23].contiguous(), Ts[:23].contiguous(), vol, 0, 2)
    with pytest.raises(_lib.HnrfError, match='24 bones'):
        _both_ways(args, 2, 128, nr_problem['c_off'], nr_problem['c_xyz'], torch.zeros(4, device=dev()), True, False)


# ------------------------------------------------------------------------------------- the canonical image
_CNL_PACK = {}


def _cnl_packed_of(seeded_params):
    if 'p' not in _CNL_PACK:
        from humannerf_amd import ops
        from humannerf_amd.seeded import default_shapes, seeded_state
        st = seeded_params if seeded_params is not None else seeded_state(default_shapes(), seed=0)
        names = [CNL + str(i) for i in range(0, 16, 2)] + ['cnl_mlp.module.output_linear.0']
        _CNL_PACK['p'] = ops.canonical_pack([G(st[n + '.weight']) for n in names], [G(st[n + '.bias']) for n in names],
                                            'f16x3')
    return _CNL_PACK['p']


# ------------------------------------------------------------------------------------- 2. the whole frame
def _share_of_the_two_kernel_sequence(net, k1_inputs, representative):
    """What the frame's share was before K1 classified: K1, then hnrf_share_compact, on the whole frame."""
    fr, Rs, Ts, vol = k1_inputs
    c_off, c_xyz = representative
    a, _ = _both_ways(_k1_args(fr, Rs, Ts, vol, 0, 576), 576, cpu.E2E_SAMPLES, c_off, c_xyz,
                      torch.zeros(4, device=dev()), True, False)
    return 1.0 - float(a['count'].item()) / float(576 * cpu.E2E_SAMPLES)


@pytest.mark.parametrize('overlap', [False, True], ids=['one_stream', 'overlap'])
@pytest.mark.parametrize('diag', [True, False], ids=['diag', 'lean'])
def test_frame_with_ragged_chunks_on_equals_off(net, frame, options, k1_inputs, diag, overlap):
    """Network.forward on the end-to-end frame in chunks of 100 rays (five whole chunks and one of 76): every output
    with the option equals the output without it, and the share of shared samples is the one K1 + hnrf_share_compact
    count on the frame's x_skel with the frame's own representative."""
    from humannerf_amd import _lib
    cfg = options
    cfg.chunk = 100
    cfg.amd.diagnostics = diag
    cfg.amd.f16_range_guard = 'audit'
    cfg.amd.overlap_warp = overlap
    cfg.amd.mlp_mode = 'f16x3'
    off, s_off = _render(net, frame, cfg, False)
    on, s_on = _render(net, frame, cfg, True)
    assert s_off == 0.0
    _assert_same(on, off, KEYS11 if diag else KEYS11[:3])
    assert float(on[-1]['alpha'].max()) > 0.1
    assert net._share_last[0].numel() == 6
    # the frame's own representative: the slot behind the two chunk workspaces (x = 0 | c_off | c_xyz | c_raw)
    ws_one = _lib.load().hnrf_render_workspace_bytes(100, cpu.E2E_SAMPLES)
    slot = net._workspace.view(torch.float32)[2 * ws_one // 4:2 * ws_one // 4 + 16].clone()
    assert bool((slot[:4] == 0).all())
    want = _share_of_the_two_kernel_sequence(net, k1_inputs, (slot[4:7].clone(), slot[8:11].clone()))
    print('shared share %s/%s: %.6f (two-kernel sequence: %.6f)' % ('diag' if diag else 'lean', overlap, s_on, want))
    assert s_on == want
    assert 0.05 < s_on < 0.95
