"""cfg.amd.share_underflow on the GPU (include/hnrf.h, hnrf_share_compact / hnrf_render_frame_shared_fwd): the non-rigid
kernel cannot tell an underflowing input from zero, the predicate kernel classifies like its numpy twin, and a frame
rendered with the option equals the frame without it bit for bit.  Everything is compared with torch.equal: the option
promises the same bits, so there is no tolerance."""
import itertools

import numpy as np
import pytest
import torch

from humannerf_amd import shared_input as si
from tests import test_shared_input_cpu as cpu

pytestmark = pytest.mark.gpu

F = np.float32
T = si.SHARE_T
NR = 'non_rigid_mlp.module.block_mlps.'
CNL = 'cnl_mlp.module.pts_linears.'


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------- 1. K2 on underflowing inputs
@pytest.fixture(scope='module')
def nr_problem(seeded_params):
    from humannerf_amd import ops
    names = [NR + str(i) for i in range(0, 14, 2)]
    ws, bs = [G(seeded_params[n + '.weight']) for n in names], [G(seeded_params[n + '.bias']) for n in names]
    cond = G((np.random.RandomState(3).randn(69) * 0.2).astype(F))
    hann = torch.ones(6, device=dev())
    packed = ops.nonrigid_pack(ws, bs, cond, 'f16x3')
    xyz0, off0 = ops.nonrigid(torch.zeros(1, 3, device=dev()), hann, packed, 'f16x3', want_offsets=True)
    return dict(packed=packed, hann=hann, c_off=off0[0].clone(), c_xyz=xyz0[0].clone())


def underflowing_inputs(P):
    """[P,3] from {+0, -0, +-1e-45, +-2^-40, +-T}: the four magnitudes, largest first, each in all eight sign patterns
    (-0 keeps its sign), then random draws of the ten values per coordinate; P = 1: one random row."""
    mags = np.array([T, 2.0 ** -40, 1e-45, 0.0], dtype=F)
    rows = np.stack([m * np.array(s, dtype=F) for m in mags for s in itertools.product((1.0, -1.0), repeat=3)])
    vals = np.concatenate([mags, -mags])
    rnd = vals[np.random.RandomState(P).randint(0, vals.size, size=(P, 3))]
    if P < 8:
        return rnd
    x = np.concatenate([rows, rnd])[:P]
    assert len({tuple(np.signbit(r)) for r in x[:8]}) == 8 and (np.abs(x[:8]) == T).all()
    return x


@pytest.mark.parametrize('mode', ['f16x3', 'f16x3+noguard'])
@pytest.mark.parametrize('P', [1, 31, 65, 257])
def test_nonrigid_kernel_sees_zero(nr_problem, P, mode):
    """Dense and sparse launches, guarded and unguarded instances: every row of offsets carries the bits of the row
    for x = (+0, +0, +0) -- condition (a) of the predicate alone decides what K2 computes; (b) is about K3's input.
    (P = 31 / 65 / 257: one lane half, both sample groups of a wave, a second workgroup with a ragged tail.)"""
    from humannerf_amd import _lib, ops
    s = nr_problem
    x = G(underflowing_inputs(P))
    want = bits(s['c_off'])[None].expand(P, 3)
    _, off = ops.nonrigid(x, s['hann'], s['packed'], mode, want_offsets=True)
    assert torch.equal(bits(off), want), 'dense'
    lib = _lib.load()
    idx = G(np.random.RandomState(P).permutation(P).astype(np.int32))
    count = torch.tensor([P], dtype=torch.int32, device=dev())
    xyz, off = torch.full((P, 3), 7.0, device=dev()), torch.full((P, 3), 7.0, device=dev())
    _lib.check(lib.hnrf_nonrigid_fwd_sparse(x.data_ptr(), s['hann'].data_ptr(), s['packed'].data_ptr(), ops._mode_arg(mode),
                                            P, idx.data_ptr(), count.data_ptr(), xyz.data_ptr(), off.data_ptr(), _stream()),
               'hnrf_nonrigid_fwd_sparse')
    assert torch.equal(bits(off), want), 'sparse'
    assert int(ops.status_word(s['packed'], 'nonrigid', 'f16x3').item()) == 0


def test_control_input_is_live(nr_problem):
    """x = 2^-20 is no underflow: the predicate, twin and kernel, calls it live (and K2's top-octave PE value 2^-15 is
    a non-zero f16)."""
    s = nr_problem
    x = np.full((1, 3), 2.0 ** -20, dtype=F)
    assert not si.shared_mask(x, s['c_off'].cpu().numpy(), s['c_xyz'].cpu().numpy())[0]
    assert np.float16(F(32.0 * 2.0 ** -20)) != 0
    idx, count, _ = _share_compact(G(x), s['c_off'], s['c_xyz'], torch.zeros(4, device=dev()), lean=True)
    assert count == 1 and idx[0] == 0


# ------------------------------------------------------------------------------------- 2. predicate kernel vs twin
def _share_compact(x, c_off, c_xyz, c_raw, lean):
    from humannerf_amd import _lib
    lib = _lib.load()
    P = x.shape[0]
    idx = torch.full((P,), -1, dtype=torch.int32, device=dev())
    count = torch.full((1,), 12345, dtype=torch.int32, device=dev())      # (the entry zeroes it)
    out = {k: torch.full((P, n), 7.0, device=dev()) for k, n in (('offsets', 3), ('xyz', 3), ('raw', 4))}
    _lib.check(lib.hnrf_share_compact(x.data_ptr(), c_off.data_ptr(), c_xyz.data_ptr(), c_raw.data_ptr(), P, idx.data_ptr(),
                                      count.data_ptr(), 0 if lean else out['offsets'].data_ptr(),
                                      0 if lean else out['xyz'].data_ptr(), out['raw'].data_ptr(), _stream()),
               'hnrf_share_compact')
    torch.cuda.synchronize()
    return idx.cpu().numpy(), int(count.item()), out


@pytest.mark.parametrize('lean', [False, True])
def test_predicate_kernel_against_twin(lean):
    x, cs = cpu.crafted_problem()
    c_raw = G(np.array([0.25, -1.5, 3.0, -0.0], dtype=F))
    for c, cx in cs:
        m = si.shared_mask(x, c, cx)
        idx, count, out = _share_compact(G(x), G(c), G(cx), c_raw, lean)
        live = si.live_indices(x, c, cx)
        assert count == live.size
        assert np.array_equal(np.sort(idx[:count]), live)          # (block order on the device: the same set)
        assert (idx[count:] == -1).all()
        sh, lv = G(m), G(~m)
        for k, want in (('raw', c_raw), ('offsets', G(c)), ('xyz', G(cx))):
            got = out[k]
            if lean and k != 'raw':
                assert bool((got == 7.0).all()), k                 # not written at all
                continue
            assert torch.equal(bits(got[sh]), bits(want)[None].expand(int(m.sum()), -1)), k
            assert bool((got[lv] == 7.0).all()), k                 # live rows are the MLPs' to write


@pytest.mark.parametrize('lean', [False, True])
def test_predicate_kernel_with_an_all_shared_block(lean):
    """P = 769: block 1 is entirely shared -- an empty block of the list, which issues no atomic -- between block 0
    (both classes), block 2 (three live samples) and block 3 (its one sample, live).  Against the numpy twin."""
    vals = np.array([0.0, -0.0, 1e-45, -1e-45, 2.0 ** -40, -2.0 ** -40], dtype=F)
    x = vals[np.random.RandomState(769).randint(0, vals.size, size=(769, 3))]   # every row shared: c absorbs these ...
    x[:256:3] = F(2.0 ** -20)                                      # ... but these: live
    x[[512 + 5, 512 + 64, 512 + 255, 768]] = F(1e-3)
    c = np.array([-0.0686608, -0.00916304, 0.06966332], F)         # an offset of the seeded network's size
    cx = (np.zeros(3, F) + c).astype(F)
    c_raw = G(np.array([0.25, -1.5, 3.0, -0.0], dtype=F))
    m = si.shared_mask(x, c, cx)
    assert m[256:512].all() and 0 < m[:256].sum() < 256 and (~m[512:768]).sum() == 3 and not m[768]
    idx, count, out = _share_compact(G(x), G(c), G(cx), c_raw, lean)
    live = si.live_indices(x, c, cx)
    assert count == live.size == 86 + 3 + 1
    assert np.array_equal(np.sort(idx[:count]), live)
    assert (idx[count:] == -1).all()
    sh, lv = G(m), G(~m)
    assert torch.equal(bits(out['raw'][sh]), bits(c_raw)[None].expand(int(m.sum()), -1))
    assert bool((out['raw'][lv] == 7.0).all())
    for k, want in (('offsets', G(c)), ('xyz', G(cx))):
        if lean:
            assert bool((out[k] == 7.0).all()), k
        else:
            assert torch.equal(bits(out[k][sh]), bits(want)[None].expand(int(m.sum()), -1)), k
            assert bool((out[k][lv] == 7.0).all()), k


# ------------------------------------------------------------------------------------- 3. end to end, on against off
KEYS11 = ('rgb', 'alpha', 'depth', 'weights_on_rays', 'rgb_on_rays', 'cnl_xyz', 'cnl_rgb', 'cnl_weight', 'xyz_on_rays',
          'backward_motion_weights', 'offsets')
AMD_KEYS = ('share_underflow', 'f16_range_guard', 'overlap_warp', 'mlp_mode', 'diagnostics', 'on_f16_range')


@pytest.fixture
def options():
    """cfg as the end-to-end frame needs it; restored afterwards."""
    from humannerf_amd.config import cfg, amd_option
    keep = (cfg.perturb, cfg.N_samples, cfg.chunk, cfg.ignore_non_rigid_motions)
    keep_amd = {k: amd_option(k) for k in AMD_KEYS}
    cfg.perturb, cfg.N_samples, cfg.chunk, cfg.ignore_non_rigid_motions = 0., cpu.E2E_SAMPLES, cpu.E2E_CHUNK, False
    yield cfg
    cfg.perturb, cfg.N_samples, cfg.chunk, cfg.ignore_non_rigid_motions = keep
    cfg.amd.update(keep_amd)


def _net(state):
    from humannerf_amd.network import Network
    net = Network()
    net.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()})
    return net.to(dev()).eval()


@pytest.fixture(scope='module')
def net(seeded_params):
    return _net(seeded_params)


@pytest.fixture(scope='module')
def frame():
    from humannerf_amd import scene
    fr = scene.synthetic_frame(**cpu.E2E_FRAME)
    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
            'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']
    return {k: G(fr[k]) for k in keys}


def _render(net, frame, cfg, share, frames=1):
    """``frames`` frames from a fresh guard schedule; returns (outputs of every frame, share of the last)."""
    cfg.amd.share_underflow = share
    net.f16_guard.restart_schedule()
    outs = []
    with torch.no_grad():
        for _ in range(frames):
            outs.append(net(**frame, iter_val=1e7))
    s = net.shared_sample_share()
    net.check_f16_range()
    return outs, s


def _assert_same(on, off, keys):
    assert len(on) == len(off)
    for a, b in zip(on, off):
        assert set(a) == set(b) == set(keys)
        for k in keys:
            assert torch.equal(bits(a[k]), bits(b[k])), k


@pytest.mark.parametrize('diag', [True, False], ids=['diag', 'lean'])
@pytest.mark.parametrize('variant', ['full', 'off', 'audit', 'overlap', 'f32'])
def test_frame_on_equals_off(net, frame, options, variant, diag):
    """All 11 outputs (the lean three) of Network.forward with the option equal those without it, bit for bit: 576
    rays x 128 samples in chunks of 128 rays (four whole chunks and one of 64), under every guard plan -- 'audit' over
    two frames: all chunks guarded, then one --, with K1 on the side stream, and in 'f32' mode, where the path is off."""
    cfg = options
    cfg.amd.diagnostics = diag
    cfg.amd.f16_range_guard = variant if variant in ('full', 'off', 'audit') else 'audit'
    cfg.amd.overlap_warp = variant == 'overlap'
    cfg.amd.mlp_mode = 'f32' if variant == 'f32' else 'f16x3'
    frames = 2 if variant == 'audit' else 1
    off, s_off = _render(net, frame, cfg, False, frames)
    on, s_on = _render(net, frame, cfg, True, frames)
    print('shared share %s/%s: %.4f' % (variant, 'diag' if diag else 'lean', s_on))
    assert s_off == 0.0
    if variant == 'f32':
        assert s_on == 0.0
    else:
        assert 0.05 < s_on < 0.95
    _assert_same(on, off, KEYS11 if diag else KEYS11[:3])
    assert float(on[-1]['alpha'].max()) > 0.1                      # (a frame with a subject in it)


# ------------------------------------------------------------------------------------- 4. extremes
def _zero_volume(net, monkeypatch):
    from humannerf_amd.config import cfg
    G_ = int(cfg.mweight_volume.volume_size)
    vol = torch.zeros(int(cfg.total_bones) + 1, G_, G_, G_, device=dev())
    monkeypatch.setattr(net, '_weight_volume', lambda priors: vol)


@pytest.mark.parametrize('diag', [True, False], ids=['diag', 'lean'])
def test_every_sample_shared(net, frame, options, monkeypatch, diag):
    """An all-zero weight volume: x_skel is exactly 0 everywhere, every live list is empty and every chunk is still
    filled and composited."""
    cfg = options
    cfg.amd.diagnostics = diag
    _zero_volume(net, monkeypatch)
    off, _ = _render(net, frame, cfg, False)
    on, s = _render(net, frame, cfg, True)
    assert s == 1.0
    assert int(net._share_last[0].sum().item()) == 0
    _assert_same(on, off, KEYS11 if diag else KEYS11[:3])


def test_hann_weight_above_one_turns_the_path_off(net, frame, options, monkeypatch):
    """The threshold assumes Hann weights <= 1: a window with a larger entry renders without the path."""
    from humannerf_amd import network
    cfg = options
    monkeypatch.setattr(network, 'hann_window_weights',
                        lambda *a: torch.tensor([1.0, 1.0, 1.5, 1.0, 1.0, 1.0], dtype=torch.float32))
    off, _ = _render(net, frame, cfg, False)
    on, s = _render(net, frame, cfg, True)
    assert s == 0.0 and net._share_last is None
    _assert_same(on, off, KEYS11)


# ------------------------------------------------------------------------------------- 5. the guard sees the class
@pytest.mark.parametrize('share', [True, False])
def test_guard_sees_the_shared_class(seeded_params, frame, options, monkeypatch, share):
    """Canonical feature 9 of layer 1 is the constant 1000 (zero weight row, zero outgoing column): out of the f16x3
    range at every input, x = 0 included.  With an all-zero weight volume every sample is shared, so with the option
    the representative's launch is the only one that can report it -- and the frame raises ActivationRangeError exactly
    as it does without the option."""
    from humannerf_amd.network import ActivationRangeError
    cfg = options
    st = {k: v.copy() for k, v in seeded_params.items() if k.startswith(CNL)}
    st[CNL + '2.weight'][9, :] = 0.0
    st[CNL + '2.bias'][9] = 1000.0
    st[CNL + '4.weight'][:, 9] = 0.0
    hot = _net(dict(seeded_params, **st))
    _zero_volume(hot, monkeypatch)
    cfg.amd.share_underflow = share
    with torch.no_grad():
        hot(**frame, iter_val=1e7)
    assert hot.shared_sample_share() == (1.0 if share else 0.0)
    with pytest.raises(ActivationRangeError, match='canonical'):
        hot.check_f16_range()
