"""View-dependent colour on the GPU (include/hnrf_view.h): the per-ray bias kernel and its backward against fp64, K4 / K4'
with the bias against the plain kernels bit for bit, the one frame entry against the four entries it stands for and
against the stage-by-stage chain, Network.forward against the reference's frames and gradients
(tests/golden/viewdir.npz) and the layered fp64 twin (tests/viewdir_cases.py), the baked path, the refusals, and every
new entry in guarded buffers.  Needs an MI355X: ``pytest -m gpu``."""
import json
import os

import numpy as np
import pytest
import torch

from tests import guarded_buffers as gb
from tests import heads_train_cases as hc
from tests import test_render_kernel_refs as refs
from tests import viewdir_cases as vc
from tests.guarded_case import T, _stream, bits, both, dev, eq, ok, same
from tests.test_grad_oracle import compare_exact, grad_frame, reference_loss

pytestmark = pytest.mark.gpu

F = np.float32
# what tests/test_gpu_grad.py::test_network_gradients_match_reference asks, and the reference's own distance from fp64
# those numbers were set against (tests/test_grad_oracle.py::test_reference_gradient_noise_floor)
REL_NORM, COS_MIN, FLOOR_NORM = 6e-3, 0.99998, 4.4e-3


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ================================================================================================ 1. the bias kernels
def embed64(dirs, L):
    """e(d) in float64 from the fp32 directions: n = d / max(|d|, 1e-12), then per band sin(2^k n), cos(2^k n)."""
    d = dirs.astype(np.float64)
    n = d / np.maximum(np.sqrt((d * d).sum(1, keepdims=True)), 1e-12)
    parts = [n]
    for k in range(L):
        parts += [np.sin(n * 2.0 ** k), np.cos(n * 2.0 ** k)]
    return np.concatenate(parts, axis=1)


def bias_problem(R, L, seed=0):
    """Directions of lengths 0.2 .. 5 with, in the first rows, a zero direction, one of length 1e3 and one of length
    1e-20; B (3, 3 + 6 L) and c (3,) of the size a folded branch has."""
    rs = np.random.RandomState(1000 * L + R + seed)
    dirs = (rs.standard_normal((R, 3)) * rs.uniform(0.2, 5.0, (R, 1))).astype(F)
    unit = np.array([0.6, -0.48, 0.64])
    special = np.stack([np.zeros(3), unit * 1e3, unit * 1e-20]).astype(F)
    dirs[:min(R, 3)] = special[:min(R, 3)]
    B = rs.uniform(-1, 1, (3, 3 + 6 * L)).astype(F)
    c = rs.uniform(-1, 1, 3).astype(F)
    return dirs, B, c, special


@pytest.mark.parametrize('L', [2, 4])
@pytest.mark.parametrize('R', [1, 63, 64, 65, 257])
def test_view_bias_forward_matches_fp64(R, L):
    """hnrf_view_bias_fwd against the numpy fp64 twin.  Bound per channel 4e-6 (sum_j |B_ij| + |c_i|): the unit direction
    carries three fp32 roundings (sum of squares, square root, division: <= 2e-7 relative), the argument 2^k n <= 8 of
    the highest band of L = 4 therefore <= 1.6e-6 absolute, sin / cos of it one more rounding: <= 2.5e-6 per term; the
    27-term fp32 sum adds 27 * 2^-24 = 1.6e-6 of the sum of magnitudes at the very most."""
    from humannerf_amd import ops
    dirs, B, c, special = bias_problem(R, L)
    cases = [dirs] if R > 1 else [special[i:i + 1].copy() for i in range(3)]       # R = 1: each special row on its own
    for d in cases:
        got = ops.view_bias(T(d), T(B), T(c)).cpu().numpy().astype(np.float64)
        want = embed64(d, L) @ B.astype(np.float64).T + c.astype(np.float64)
        bound = 4e-6 * (np.abs(B).astype(np.float64).sum(1) + np.abs(c))
        err = np.abs(got - want).max(0)
        print('view_bias R', d.shape[0], 'L', L, 'err / bound', (err / bound).max())
        assert (err <= bound).all(), (err, bound)
    # the zero direction: e = (0, sin 0, cos 0, ...) exactly
    z = ops.view_bias(T(np.zeros((1, 3), F)), T(B), T(c)).cpu().numpy()[0].astype(np.float64)
    cos_cols = [3 + 6 * k + 3 + a for k in range(L) for a in range(3)]
    assert np.abs(z - (c.astype(np.float64) + B[:, cos_cols].astype(np.float64).sum(1))).max() <= 1e-6 * (np.abs(B).sum(1) + 1).max()


@pytest.mark.parametrize('L', [2, 4])
@pytest.mark.parametrize('R', [1, 65, 6144])
def test_view_bias_backward_matches_fp64_and_repeats_its_bits(R, L):
    """hnrf_view_bias_bwd against dB = d_bias^T e(d), dc = sum d_bias in fp64.  Bound per entry
    (2.5e-6 + depth 2^-24) sum_r |d_bias_ri|: every term d_bias e carries e's error (the forward's 2.5e-6, |e| <= 1) and
    one product rounding, and the two-stage sum is ``depth`` fp32 additions deep -- the trips of a thread's loop, 6
    butterfly steps, 3 waves, the slices, and the product -- each at most 2^-24 of the sum of magnitudes.  No atomics: a
    second call returns the same bits."""
    from humannerf_amd import ops
    dirs, _, _, _ = bias_problem(R, L, seed=7)
    rs = np.random.RandomState(R + L)
    d_bias = (rs.standard_normal((R, 3)) * (rs.uniform(size=(R, 1)) > 0.3)).astype(F)
    dB, dc = ops.view_bias_bwd(T(dirs), T(d_bias), L)
    dB2, dc2 = ops.view_bias_bwd(T(dirs), T(d_bias), L)
    assert same_bits(dB, dB2) and same_bits(dc, dc2)
    e = embed64(dirs, L)
    want_B, want_c = d_bias.astype(np.float64).T @ e, d_bias.astype(np.float64).sum(0)
    slices = min(64, -(-R // 256))
    depth = -(-R // (256 * slices)) + 6 + 3 + slices + 1
    bound = (2.5e-6 + depth * 2.0 ** -24) * np.abs(d_bias).astype(np.float64).sum(0)
    err_B = np.abs(dB.cpu().numpy() - want_B).max(1)
    err_c = np.abs(dc.cpu().numpy() - want_c)
    print('view_bias_bwd R', R, 'L', L, 'err / bound', (err_B / np.maximum(bound, 1e-300)).max(), (err_c / np.maximum(bound, 1e-300)).max())
    assert (err_B <= bound).all() and (err_c <= bound).all(), (err_B, err_c, bound)
    assert tuple(dB.shape) == (3, 3 + 6 * L) and tuple(dc.shape) == (3,)


def test_view_bias_autograd_function():
    """autograd.ViewBias: B and c receive hnrf_view_bias_bwd's gradients, the directions none."""
    from humannerf_amd.autograd import ViewBias
    from humannerf_amd import ops
    dirs, B, c, _ = bias_problem(65, 4)
    Bt, ct, dt = T(B).requires_grad_(True), T(c).requires_grad_(True), T(dirs).requires_grad_(True)
    out = ViewBias.apply(dt, Bt, ct)
    assert same_bits(out.detach(), ops.view_bias(T(dirs), T(B), T(c)))
    g = T(np.random.RandomState(1).standard_normal((65, 3)).astype(F))
    out.backward(g)
    dB, dc = ops.view_bias_bwd(T(dirs), g, 4)
    assert same_bits(Bt.grad, dB) and same_bits(ct.grad, dc) and dt.grad is None


# ================================================================================================ 2. K4 / K4' with the bias
K4_S = [2, 63, 64, 65, 128, 130]
K4_R = [1, 5]


def k4_case(R, S):
    c4 = refs.k4_problem(R, S, 'sparse')
    rs = np.random.RandomState(10 * S + R)
    c4['bias'] = (rs.standard_normal((R, 3)) * 1.5).astype(F)
    return c4


def pre_added(raw, bias):
    """raw with the per-ray bias added to its colour channels, one fp32 add per value (on the device, as the kernel)."""
    out = raw.clone()
    out[..., :3] += bias[:, None, :]
    return out


@pytest.mark.parametrize('cull_eps', [0.0, refs.K4_CULL_EPS])
@pytest.mark.parametrize('diag', [False, True], ids=['lean', 'diag'])
@pytest.mark.parametrize('R', K4_R)
@pytest.mark.parametrize('S', K4_S)
def test_composite_view_forward(S, R, diag, cull_eps):
    """hnrf_composite_view_fwd: with a null or an all-zero bias bit-equal to hnrf_composite_fwd on every output; with a
    seeded bias bit-equal to hnrf_composite_fwd on raw with the bias pre-added in fp32 (one fp32 add either way)."""
    from humannerf_amd import ops
    c4 = k4_case(R, S)
    a = [T(c4[k]) for k in ('mask', 'z', 'rays_d')]
    raw, xyz, bg, bias = T(c4['raw']), T(c4['xyz']), T(c4['bg']), T(c4['bias'])
    kw = dict(diagnostics=diag, cull_eps=cull_eps)
    plain = ops.composite(raw, *a, xyz if diag else None, bg, **kw)
    assert len(plain) == (8 if diag else 3)
    zero = ops.composite(raw, *a, xyz if diag else None, bg, view_bias=torch.zeros_like(bias), **kw)
    for k in plain:
        assert same_bits(zero[k], plain[k]), k
    got = ops.composite(raw, *a, xyz if diag else None, bg, view_bias=bias, **kw)
    want = ops.composite(pre_added(raw, bias), *a, xyz if diag else None, bg, **kw)
    for k in want:
        assert same_bits(got[k], want[k]), k
    assert not same_bits(got['rgb'], plain['rgb'])                  # (the bias does something)
    # the null pointer through the C entry itself
    from humannerf_amd import _lib
    lib = _lib.load_view()
    out = {k: torch.empty_like(v) for k, v in plain.items()}
    g = lambda k: None if k not in out else out[k].data_ptr()
    ok(lib.hnrf_composite_view_fwd(raw.data_ptr(), a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(),
                                   xyz.data_ptr() if diag else None, bg.data_ptr(), None, R, S, cull_eps, g('rgb'), g('alpha'),
                                   g('depth'), g('weights_on_rays'), g('rgb_on_rays'), g('cnl_xyz'), g('cnl_rgb'),
                                   g('cnl_weight'), _stream()), 'hnrf_composite_view_fwd')
    for k in plain:
        assert same_bits(out[k], plain[k]), k


@pytest.mark.parametrize('R', K4_R)
@pytest.mark.parametrize('S', K4_S)
def test_composite_view_backward(S, R):
    """hnrf_composite_view_bwd: d_raw and d_mask bit-equal to hnrf_composite_bwd on the pre-added raw; d_bias against
    the fp64 sum of d_raw.xyz over the ray's samples within S 2^-24 sum_s |d_raw| (at most S additions in any order)."""
    from humannerf_amd import ops
    c4 = k4_case(R, S)
    from tests.test_train_kernel_refs import composite_problem
    cp = composite_problem(R, S, 'sparse')
    a = [T(c4[k]) for k in ('mask', 'z', 'rays_d')]
    raw, bg, bias = T(c4['raw']), T(c4['bg']), T(c4['bias'])
    g = [T(cp['g_rgb']), T(cp['g_a']), T(cp['g_d'])]
    d_raw, d_mask, d_bias = ops.composite_bwd(raw, *a, bg, *g, view_bias=bias)
    w_raw, w_mask = ops.composite_bwd(pre_added(raw, bias), *a, bg, *g)
    assert same_bits(d_raw, w_raw) and same_bits(d_mask, w_mask)
    p_raw, p_mask = ops.composite_bwd(raw, *a, bg, *g)
    z_raw, z_mask, _ = ops.composite_bwd(raw, *a, bg, *g, view_bias=torch.zeros_like(bias))
    assert same_bits(z_raw, p_raw) and same_bits(z_mask, p_mask)
    assert not same_bits(d_raw, p_raw)
    d64 = d_raw.cpu().numpy().astype(np.float64)[..., :3]
    err = np.abs(d_bias.cpu().numpy() - d64.sum(1))
    bound = S * 2.0 ** -24 * np.abs(d64).sum(1)
    assert (err <= bound).all(), (err.max(), bound.min())
    assert float(np.abs(d64).sum()) > 0
    # rgb alone (g_alpha, g_depth null), as the trainer's loss has it
    o_raw, o_mask, o_bias = ops.composite_bwd(raw, *a, bg, g[0], view_bias=bias)
    q_raw, q_mask = ops.composite_bwd(pre_added(raw, bias), *a, bg, g[0])
    assert same_bits(o_raw, q_raw) and same_bits(o_mask, q_mask) and tuple(o_bias.shape) == (R, 3)


# ================================================================================================ 3. the frame entry
FRAME_S, FRAME_CHUNK = 16, 64


@pytest.fixture(scope='module')
def plain_parts(seeded_params, golden_dir):
    """K1's inputs, both packed images (f16x3), the Hann weights and the two grids for the fixture's 200 rays, from a
    single-head Network on the seeded state with sigma at the fixture's scale."""
    from humannerf_amd import ops
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network, hann_window_weights
    from humannerf_amd.seeded import with_density
    fr = vc.fixture_frame(golden_dir)
    net = Network()
    state = dict(seeded_params)
    w, b = state['cnl_mlp.module.output_linear.0.weight'].copy(), state['cnl_mlp.module.output_linear.0.bias'].copy()
    w[3], b[3] = w[3] * F(vc.SIGMA_SCALE), b[3] * F(vc.SIGMA_SCALE)
    state['cnl_mlp.module.output_linear.0.weight'], state['cnl_mlp.module.output_linear.0.bias'] = w, b
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    net = net.to(dev()).eval()
    d = {k: T(fr[k]) for k in vc.FRAME_KEYS}
    keep = cfg.amd.mlp_mode
    cfg.amd.mlp_mode = 'f16x3'
    try:
        with torch.no_grad():
            Rs, Ts, vol = net.frame_motion(fr)
            nrc = cfg.non_rigid_motion_mlp
            hann_w = hann_window_weights(1e7, nrc.multires, nrc.kick_in_iter, nrc.full_band_iter).to(dev())
            nr_packed = net._nonrigid_packed(d['dst_posevec']).clone()
            cnl_packed = net._canonical_packed().clone()
    finally:
        cfg.amd.mlp_mode = keep
    k1 = (d['rays'][0].contiguous(), d['rays'][1].contiguous(), d['near'].reshape(-1), d['far'].reshape(-1), None, Rs, Ts,
          vol, d['cnl_bbox_min_xyz'], d['cnl_bbox_scale_xyz'])
    lo, hi = d['cnl_bbox_min_xyz'], T(fr['cnl_bbox_max_xyz'])
    grid = ops.bake_canonical(cnl_packed, lo, hi, 24, 'f16x3')
    off = ops.bake_nonrigid(nr_packed, hann_w, lo, hi, 16, 'f16x3')
    bias = T((np.random.RandomState(11).standard_normal((vc.N_RAYS, 3)) * 1.5).astype(F))
    torch.cuda.synchronize()
    return dict(k1=k1, hann_w=hann_w, nr=nr_packed, cnl=cnl_packed, bg=d['bgcolor'], grid=(grid, lo, hi), off=(off, lo, hi),
                bias=bias, B=net.total_bones)


PATHS = {'exact': {}, 'shared': {'share': True}, 'baked': {'baked': True}, 'baked_nr': {'baked': True, 'baked_nr': True}}


def frame_call(p, path, diag, view_bias=None, chunk=FRAME_CHUNK):
    from humannerf_amd import ops
    kw = {}
    if PATHS[path].get('baked'):
        kw['baked'] = p['grid']
    if PATHS[path].get('baked_nr'):
        kw['baked_nr'] = p['off']
    if PATHS[path].get('share'):
        kw['share_log'] = []
    if view_bias is not None:
        kw['view_bias'] = view_bias
    out, _ = ops.render_frame(*p['k1'], p['hann_w'], p['nr'], p['cnl'], p['bg'], FRAME_S, chunk, 'f16x3', diagnostics=diag,
                              overlap=False, **kw)
    return out


@pytest.mark.parametrize('diag', [True, False], ids=['diag', 'lean'])
@pytest.mark.parametrize('path', list(PATHS))
def test_frame_entry_with_zero_bias_equals_the_entry_it_stands_for(path, diag, plain_parts):
    """hnrf_render_frame_view_fwd with B = 0 (an all-zero bias) on the single-head image is bit-equal to
    hnrf_render_frame_fwd / _shared_fwd / _baked_fwd / _baked_nr_fwd on every output -- all 11 with the diagnostics --:
    200 rays in chunks of 64, three full chunks and a tail of 8."""
    p = plain_parts
    want = frame_call(p, path, diag)
    got = frame_call(p, path, diag, view_bias=torch.zeros_like(p['bias']))
    assert set(got) == set(want) and len(want) == (11 if diag else 3)
    for k in want:
        assert same_bits(got[k], want[k]), (path, k)
    assert float(want['alpha'].max()) > 0.05                        # (something is rendered)


@pytest.mark.parametrize('diag', [True, False], ids=['diag', 'lean'])
@pytest.mark.parametrize('path', list(PATHS))
def test_frame_entry_with_a_seeded_bias_is_the_chain_of_its_stages(path, diag, plain_parts):
    """The frame with a seeded per-ray bias is bit-equal to the stage-by-stage chain sample_warp -> nonrigid -> canonical
    -> composite(view_bias=...) (the baked paths: the grid samplers in the MLPs' places), chunk after chunk."""
    from humannerf_amd import ops
    p = plain_parts
    got = frame_call(p, path, diag, view_bias=p['bias'])
    z, x_skel, mask, bmw = ops.sample_warp(*p['k1'], FRAME_S, want_bmw=diag)
    if path == 'baked_nr':
        raw, xyz, off = ops.baked_warp_sample(x_skel, p['off'], p['grid'], want_xyz=True, want_offsets=True)
    else:
        xyz, off = ops.nonrigid(x_skel, p['hann_w'], p['nr'], 'f16x3', want_offsets=True)
        raw = ops.baked_sample(xyz, *p['grid']) if path == 'baked' else ops.canonical(xyz, p['cnl'], 'f16x3')
    ref = ops.composite(raw, mask, z, p['k1'][1], xyz, p['bg'], diagnostics=diag, view_bias=p['bias'])
    if diag:
        ref.update(xyz_on_rays=xyz, backward_motion_weights=bmw, offsets=off)
    assert set(got) == set(ref)
    for k in ref:
        assert same_bits(got[k], ref[k]), (path, k)
    assert not same_bits(got['rgb'], frame_call(p, path, diag)['rgb'])


# ================================================================================================ 4. Network.forward
@pytest.fixture(scope='module')
def fixture_npz(golden_dir):
    return np.load(os.path.join(golden_dir, 'viewdir.npz'))


def view_network(state, train=False):
    from humannerf_amd.network import Network
    net = Network()
    assert net.view_bands == vc.BANDS
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    net = net.to(dev())
    return net.train() if train else net.eval()


@pytest.mark.parametrize('camera_only', [False, True])
@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
def test_frame_matches_the_reference(mode, camera_only, seeded_params, golden_dir, fixture_npz):
    """Network.forward against the reference's Network.forward on the fixture's 200 rays (S = 16, chunks of 64: three
    full ones and a tail of 8), for both view_dir_camera_only settings.  Tolerances: the golden cases' own, rgb / alpha
    2e-5 and depth 1e-4 far, as tests/test_gpu_multihead.py uses them."""
    fr = vc.fixture_frame(golden_dir)
    data = {k: T(fr[k]) for k in vc.FRAME_KEYS}
    with vc.view_config(camera_only=camera_only, N_samples=vc.FIXTURE_S, chunk=FRAME_CHUNK, mlp_mode=mode,
                        diagnostics=True), torch.no_grad():
        net = view_network(vc.view_state(seeded_params))
        out = net(**data, iter_val=1e7)
        assert net.check_f16_range(wait=True) is False
        lean_cfg = vc.view_config(camera_only=camera_only, N_samples=vc.FIXTURE_S, chunk=FRAME_CHUNK, mlp_mode=mode,
                                  diagnostics=False)
        with lean_cfg:
            lean = net(**data, iter_val=1e7)
    i = int(camera_only)
    far = float(fr['far'].max())
    for k, tol in (('rgb', 2e-5), ('alpha', 2e-5), ('depth', 1e-4 * far)):
        err = np.abs(out[k].cpu().numpy() - fixture_npz[k][i]).max()
        print('frame', mode, 'camera_only', camera_only, k, 'err vs reference %.2e' % err)
        assert err <= tol, (k, err)
        assert same_bits(lean[k], out[k]), k
    assert len(out) == 11 and len(lean) == 3
    # the two settings differ in the fixture, so a frame that ignored the third row could not pass both
    assert np.abs(fixture_npz['rgb'][1] - fixture_npz['rgb'][0]).max() > 1e-2


def test_shared_underflow_path_keeps_its_bits_with_view_colour(seeded_params, golden_dir):
    """cfg.amd.share_underflow on and off render the same bits with view colour (the bias is K4's, behind the sharing)."""
    fr = vc.fixture_frame(golden_dir)
    data = {k: T(fr[k]) for k in vc.FRAME_KEYS}
    outs = []
    for share in (False, True):
        with vc.view_config(N_samples=vc.FIXTURE_S, chunk=FRAME_CHUNK, mlp_mode='f16x3', diagnostics=True,
                            share_underflow=share), torch.no_grad():
            net = view_network(vc.view_state(seeded_params))
            outs.append(net(**data, iter_val=1e7))
            assert (net._share_last is not None) == share
    for k in outs[0]:
        assert same_bits(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize('nonrigid', ['mlp', 'baked'])
def test_baked_path_with_view_colour(nonrigid, seeded_params, golden_dir):
    """cfg.amd.canonical = 'baked' with view colour: the grid is that of the folded image baked WITHOUT a view (a pure
    function of position), and the frame equals compositing the grid sampler's raw with the per-ray bias, bit for bit."""
    from humannerf_amd import ops
    fr = vc.fixture_frame(golden_dir)
    data = {k: T(fr[k]) for k in vc.FRAME_KEYS}
    data['cnl_bbox_max_xyz'] = T(fr['cnl_bbox_max_xyz'])
    with vc.view_config(N_samples=vc.FIXTURE_S, chunk=FRAME_CHUNK, mlp_mode='f16x3', diagnostics=True, canonical='baked',
                        nonrigid=nonrigid, bake_resolution=24, nonrigid_bake_resolution=16), torch.no_grad():
        net = view_network(vc.view_state(seeded_params))
        net.fixed_view((0.0, 0.0, 1.0))                             # (a chosen direction must not reach the renderer's grid)
        out = net(**data, iter_val=1e7)
        kept = net._kept['baked']
        hw, hb, B, zero3 = net._view_fold()
        lin = net.cnl_mlp.module.trunk()
        folded = ops.canonical_pack([l.weight.detach() for l in lin] + [hw], [l.bias.detach() for l in lin] + [hb], 'f16x3')
        grid = ops.bake_canonical(folded, kept.bmin, kept.bmax, 24, 'f16x3')
        assert same_bits(kept.grid.view(torch.int16), grid.view(torch.int16)) and kept.key[-1] is None
        bias = ops.view_bias(data['rays'][1].contiguous(), B, zero3)
        Rs, Ts, vol = net.frame_motion(fr)
        z, x_skel, mask, _ = ops.sample_warp(data['rays'][0].contiguous(), data['rays'][1].contiguous(), data['near'].reshape(-1),
                                             data['far'].reshape(-1), None, Rs, Ts, vol, data['cnl_bbox_min_xyz'],
                                             data['cnl_bbox_scale_xyz'], vc.FIXTURE_S)
        if nonrigid == 'baked':
            nr = net._kept['baked_nr']
            raw, xyz, _ = ops.baked_warp_sample(x_skel, (nr.grid, nr.bmin, nr.bmax), (grid, kept.bmin, kept.bmax),
                                                want_xyz=True, want_offsets=True)
        else:
            xyz = out['xyz_on_rays'].reshape(x_skel.shape).contiguous()
            raw = ops.baked_sample(xyz, grid, kept.bmin, kept.bmax)
        ref = ops.composite(raw, mask, z, data['rays'][1].contiguous(), xyz, data['bgcolor'], diagnostics=True, view_bias=bias)
        for k in ref:
            assert same_bits(out[k], ref[k]), k
        # a direct bake takes fixed_view's direction, and is another grid
        direct = net.bake_canonical(data['cnl_bbox_min_xyz'], data['cnl_bbox_max_xyz'], 24)
        assert net._kept['baked'].key[-1] == (0.0, 0.0, 1.0)
        assert not torch.equal(direct[..., :3], grid[..., :3]) and torch.equal(direct[..., 3], grid[..., 3])


def test_fixed_view_colours_and_refusals(seeded_params, golden_dir):
    """vertex_colors seen from fixed_view's direction against the layered fp64 twin (2e-5, the golden cases' bound on a
    colour); without a direction it raises; cfg.amd.term_eps > 0 and camera-only with a two-row ``rays`` are refused."""
    from oracle import oracle
    fr = vc.fixture_frame(golden_dir)
    data = {k: T(fr[k]) for k in vc.FRAME_KEYS}
    state = vc.view_state(seeded_params)
    with vc.view_config(N_samples=vc.FIXTURE_S, chunk=FRAME_CHUNK, mlp_mode='f32', diagnostics=False) as cfg, torch.no_grad():
        net = view_network(state)
        pts = np.random.RandomState(2).uniform(-0.8, 0.8, (257, 3)).astype(F)
        with pytest.raises(RuntimeError, match='fixed_view'):
            net.vertex_colors(T(pts))
        d0 = (0.3, -2.0, 1.1)
        got = net.fixed_view(d0).vertex_colors(T(pts)).cpu().numpy()
        dirs = torch.tensor(d0, dtype=torch.float64).expand(257, 3)
        raw = vc.canonical_view_raw(vc.t64(state, 'cnl_mlp'), oracle.fourier_pe(torch.from_numpy(pts).double(), 10), dirs)
        err = np.abs(got - torch.sigmoid(raw[:, :3]).numpy()).max()
        print('vertex colours from a fixed view: err vs fp64 %.2e' % err)
        assert err <= 2e-5
        other = net.fixed_view((0.0, 1.0, 0.0)).vertex_colors(T(pts)).cpu().numpy()
        assert np.abs(other - got).max() > 1e-3
        net.fixed_view(None)
        cfg.amd.term_eps = 1e-3
        try:
            with pytest.raises(NotImplementedError, match='term_eps'):
                net(**data, iter_val=1e7)
        finally:
            cfg.amd.term_eps = 0.0
        cfg.canonical_mlp.view_dir_camera_only = True
        with pytest.raises(ValueError, match='view_dir_camera_only'):
            net(**dict(data, rays=data['rays'][:2].contiguous()), iter_val=1e7)


# ================================================================================================ 5. gradients
@pytest.fixture(scope='module')
def grad_case(seeded_params, golden_dir):
    with open(os.path.join(golden_dir, 'meta.json')) as f:
        meta = json.load(f)['grad_s64']
    state = vc.view_state(seeded_params, sigma_scale=vc.TRAIN_SIGMA_SCALE)
    fr = vc.with_camera_row(grad_frame(meta))
    lw = hc.head_loss_weights(meta['n_rays'])[0]
    exact, _ = vc.gradients(state, fr, lw, iter_val=meta['iter_val'], N_samples=meta['N_samples'])
    return dict(meta=meta, state=state, fr=fr, lw=lw, exact=exact)


@pytest.mark.parametrize('train_mode,operands', [('f32', 'f32'), ('f16x3', 'f32'), ('f16x3', 'f16')])
def test_view_gradients_match_reference(train_mode, operands, grad_case, fixture_npz):
    """A training-mode forward with view colour in the three arithmetic settings of
    tests/test_gpu_grad.py::test_network_gradients_match_reference, against the reference's own loss.backward() (the
    fixture) and against fp64 autograd through the layered twin -- all 61 tensors, the four view layers among them: their
    gradients arrive through the fold.  Bounds: that test's, 6e-3 in norm and cosine 0.99998 (pose decoder against fp64:
    1e-2 / 0.99997), scaled by the recorded floor / 4.4e-3 when the reference's own recorded distance from fp64 is larger
    (recorded with the fixture: 1.9e-3, so they hold as they stand)."""
    from humannerf_amd.network import full_gradient
    meta, g = grad_case['meta'], fixture_npz
    data = {k: T(grad_case['fr'][k]) for k in vc.FRAME_KEYS}
    with vc.view_config(N_samples=meta['N_samples'], train_mlp_mode=train_mode, train_dw_mode=train_mode,
                        train_chain_mode=train_mode, train_operands=operands, diagnostics=True):
        net = view_network(grad_case['state'], train=True)
        out = net(**data, iter_val=meta['iter_val'])
        assert len(out) == 11 and not out['weights_on_rays'].requires_grad and out['rgb'].requires_grad
        loss = reference_loss(out, torch.from_numpy(grad_case['lw']).to(dev()))
        loss.backward()
    print('loss', float(loss), 'reference', float(g['loss']))
    assert abs(float(loss) - float(g['loss'])) <= 2e-4 * max(1.0, abs(float(g['loss'])))
    grads = {k: (full_gradient(p).cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
             for k, p in net.named_parameters()}
    assert len(grads) == 61
    for layer in vc.VIEW_LAYERS:
        assert float(np.abs(grads[vc.P + layer + '.weight']).max()) > 0 and float(np.abs(grads[vc.P + layer + '.bias']).max()) > 0
    r = c = max(1.0, float(g['noise_floor']) / FLOOR_NORM)
    print('bounds: norm %.3e cosine %.6f (recorded floor %.2e / %.7f)'
          % (REL_NORM * r, 1.0 - (1.0 - COS_MIN) * c, float(g['noise_floor']), float(g['noise_floor_cos'])))
    vs_exact = compare_exact(grads, grad_case['exact'], rel_norm=REL_NORM * r, cos_min=1.0 - (1.0 - COS_MIN) * c,
                             loose=('pose_decoder.', 1e-2 * r, 1.0 - 3e-5 * c))
    print(train_mode, operands, '| vs fp64', vs_exact)
    vs_ref = vc.compare_to_fixture(grads, g, rel_norm=REL_NORM * r, cos_min=1.0 - (1.0 - COS_MIN) * c, n_tensors=61)
    print(train_mode, operands, '| vs reference', vs_ref)


def test_training_forward_equals_the_inference_render(grad_case):
    """The training-mode forward (fp32 fold under autograd, exact-fp32 kernels) and the inference render (fp64 fold
    rounded once) of the same weights agree to the golden cases' bound, and positional RenderRays calls without a bias
    keep working."""
    meta = grad_case['meta']
    data = {k: T(grad_case['fr'][k]) for k in vc.FRAME_KEYS}
    with vc.view_config(N_samples=meta['N_samples'], train_mlp_mode='f32', train_dw_mode='f32', train_chain_mode='f32',
                        train_operands='f32', mlp_mode='f32', diagnostics=False):
        net = view_network(grad_case['state'], train=True)
        out = net(**data, iter_val=meta['iter_val'])
        with torch.no_grad():
            ref = net.eval()(**data, iter_val=meta['iter_val'])
    for k in ('rgb', 'alpha'):
        err = float((out[k].detach() - ref[k]).abs().max())
        print('training forward vs inference', k, '%.2e' % err)
        assert err <= 2e-5, (k, err)


# ================================================================================================ 6. buffer bounds
R0, S0 = 37, 21


@pytest.mark.parametrize('L', [1, 4, 10])
def test_bias_entries_stay_inside_their_buffers(L):
    """hnrf_view_bias_fwd / _bwd with every buffer guarded at exactly the stated size, under both fills: guards intact,
    outputs bit-equal between the fills and to the ops wrapper, inputs unchanged; R = 0 writes no bias, and dB / dc whole
    zeros."""
    from humannerf_amd import _lib, ops
    lib = _lib.load_view()
    E = 3 + 6 * L
    for R in (R0, 300):
        dirs, B, c, _ = bias_problem(R, L)
        d_bias = np.random.RandomState(R).standard_normal((R, 3)).astype(F)

        def fwd(k):
            ok(lib.hnrf_view_bias_fwd(k.put('dirs', dirs), k.put('B', B), k.put('c', c), L, R, k.new('bias', 12 * R),
                                      _stream()), 'hnrf_view_bias_fwd')
        a, b = both(fwd)
        same(a, b, ['bias'])
        eq(a, 'bias', ops.view_bias(T(dirs), T(B), T(c)))
        need = lib.hnrf_view_bias_bwd_workspace_bytes(R, L)
        assert need == -(-(min(64, -(-R // 256)) * (E + 1) * 12) // 256) * 256

        def bwd(k):
            ok(lib.hnrf_view_bias_bwd(k.put('dirs', dirs), k.put('d_bias', d_bias), L, R, k.new('ws', need), need,
                                      k.new('dB', 12 * E), k.new('dc', 12), _stream()), 'hnrf_view_bias_bwd')
        a, b = both(bwd)
        same(a, b, ['dB', 'dc'])
        dB, dc = ops.view_bias_bwd(T(dirs), T(d_bias), L)
        eq(a, 'dB', dB)
        eq(a, 'dc', dc)

    def empty(k):
        ok(lib.hnrf_view_bias_fwd(k.put('dirs', np.zeros((1, 3), F)), k.put('B', B), k.put('c', c), L, 0, k.new('bias', 12),
                                  _stream()), 'hnrf_view_bias_fwd')
        need = lib.hnrf_view_bias_bwd_workspace_bytes(0, L)
        ok(lib.hnrf_view_bias_bwd(k.put('d', np.zeros((1, 3), F)), k.put('g', np.zeros((1, 3), F)), L, 0, k.new('ws', need),
                                  need, k.new('dB', 12 * E), k.new('dc', 12), _stream()), 'hnrf_view_bias_bwd')
    a, b = both(empty)
    a.g['bias'].holds_fill(), b.g['bias'].holds_fill()
    for k in (a, b):
        assert float(k.f('dB').abs().max()) == 0.0 and float(k.f('dc').abs().max()) == 0.0
    # refused before any launch: a short or misaligned workspace, bands out of range
    def refused(k):
        need = lib.hnrf_view_bias_bwd_workspace_bytes(R0, L)
        args = lambda ws, nbytes, bands: (k.put('dirs', dirs[:R0]), k.put('d_bias', d_bias[:R0]), bands, R0, ws, nbytes,
                                          k.new('dB', 12 * E), k.new('dc', 12), _stream())
        assert lib.hnrf_view_bias_bwd(*args(k.new('ws', need), need - 1, L)) == -4
        assert lib.hnrf_view_bias_bwd(*args(k.new('ws', need + 4, misalign=4), need, L)) == -1
        assert lib.hnrf_view_bias_bwd(*args(k.new('ws', need), need, 11)) == -1
        assert lib.hnrf_view_bias_fwd(k.put('dirs', dirs[:R0]), k.put('B', B), k.put('c', c), 0, R0, k.new('bias', 12 * R0),
                                      _stream()) == -1
    a, b = both(refused)
    for k in (a, b):
        for name in ('dB', 'dc', 'ws', 'bias'):
            k.g[name].holds_fill()


@pytest.mark.parametrize('diag', [False, True], ids=['lean', 'diag'])
@pytest.mark.parametrize('S', [2, S0, 65, 512])
def test_composite_view_entries_stay_inside_their_buffers(S, diag):
    """hnrf_composite_view_fwd / _bwd in guarded buffers (the bias of exactly 12 R bytes): guards intact, outputs
    bit-equal between the fills and to the ops wrapper."""
    from humannerf_amd import _lib, ops
    from tests.test_train_kernel_refs import composite_problem
    lib = _lib.load_view()
    R = R0
    c4 = k4_case(R, S)
    cp = composite_problem(R, S, 'sparse')
    per = {'rgb': 3, 'alpha': 1, 'depth': 1, 'weights_on_rays': S, 'rgb_on_rays': 3 * S, 'cnl_xyz': 3, 'cnl_rgb': 3,
           'cnl_weight': 1}
    names = list(per)[:8 if diag else 3]

    def fwd(k):
        outs = [k.new(n, 4 * R * per[n]) for n in names] + [None] * (0 if diag else 5)
        ok(lib.hnrf_composite_view_fwd(k.put('raw', c4['raw']), k.put('mask', c4['mask']), k.put('z', c4['z']),
                                       k.put('rays_d', c4['rays_d']), k.put('xyz', c4['xyz']) if diag else None,
                                       k.put('bg', c4['bg']), k.put('bias', c4['bias']), R, S, 0.0, *outs, _stream()),
           'hnrf_composite_view_fwd')
    a, b = both(fwd)
    same(a, b, names)
    want = ops.composite(T(c4['raw']), T(c4['mask']), T(c4['z']), T(c4['rays_d']), T(c4['xyz']) if diag else None, T(c4['bg']),
                         diagnostics=diag, view_bias=T(c4['bias']))
    for n in names:
        eq(a, n, want[n])
    if diag:
        return

    def bwd(k):
        ok(lib.hnrf_composite_view_bwd(k.put('raw', c4['raw']), k.put('mask', c4['mask']), k.put('z', c4['z']),
                                       k.put('rays_d', c4['rays_d']), k.put('bg', c4['bg']), k.put('bias', c4['bias']),
                                       k.put('g_rgb', cp['g_rgb']), k.put('g_a', cp['g_a']), k.put('g_d', cp['g_d']), R, S,
                                       k.new('d_raw', 16 * R * S), k.new('d_mask', 4 * R * S), k.new('d_bias', 12 * R),
                                       _stream()), 'hnrf_composite_view_bwd')
    a, b = both(bwd)
    same(a, b, ['d_raw', 'd_mask', 'd_bias'])
    d_raw, d_mask, d_bias = ops.composite_bwd(T(c4['raw']), T(c4['mask']), T(c4['z']), T(c4['rays_d']), T(c4['bg']),
                                              T(cp['g_rgb']), T(cp['g_a']), T(cp['g_d']), view_bias=T(c4['bias']))
    eq(a, 'd_raw', d_raw)
    eq(a, 'd_mask', d_mask)
    eq(a, 'd_bias', d_bias)


@pytest.mark.parametrize('diag', [True, False], ids=['diag', 'lean'])
@pytest.mark.parametrize('path', list(PATHS))
def test_frame_view_entry_stays_inside_its_buffers(path, diag, plain_parts):
    """hnrf_render_frame_view_fwd called directly with the bias (12 N bytes), every output and a workspace of exactly the
    stated size in guarded buffers: guards intact, outputs bit-equal between the fills and to the ops wrapper; a workspace
    one byte short and an offset grid without a canonical grid are refused with everything left at the fill."""
    from humannerf_amd import _lib, ops
    lib = _lib.load_view()
    p = plain_parts
    N, S, B, G, chunk = vc.N_RAYS, FRAME_S, p['B'], p['k1'][7].shape[-1], FRAME_CHUNK
    share = bool(PATHS[path].get('share'))
    need = (lib.hnrf_render_frame_shared_workspace_bytes if share else lib.hnrf_render_frame_workspace_bytes)(chunk, S)
    shapes = ops.output_shapes(S, B, diag)
    sizes = {k: 4 * N * int(np.prod(v)) for k, v in shapes.items()}
    grid = [p['grid'][0].data_ptr(), p['grid'][0].shape[0], p['grid'][1].data_ptr(), p['grid'][2].data_ptr()] \
        if PATHS[path].get('baked') else [None, 0, None, None]
    off = [p['off'][0].data_ptr(), p['off'][0].shape[0], p['off'][1].data_ptr(), p['off'][2].data_ptr()] \
        if PATHS[path].get('baked_nr') else [None, 0, None, None]
    ptr = lambda t: None if t is None else t.data_ptr()
    n_chunks = -(-N // chunk)

    def call(k, ws_bytes=need, off_args=off, grid_args=grid):
        outs = [k.new(n, sizes[n]) if n in sizes else None for n in ops.output_shapes(S, B)]
        live = k.new('live', 4 * n_chunks) if share else None
        return lib.hnrf_render_frame_view_fwd(
            *[ptr(t) for t in p['k1']], ptr(p['hann_w']), ptr(p['nr']), ptr(p['cnl']), *off_args, *grid_args,
            k.put('bias', p['bias']), ptr(p['bg']), ops._mode_arg('f16x3'), 0.0, N, S, B, G, chunk, k.new('ws', need), ws_bytes,
            *outs, live, None, None, None, _stream())
    a, b = both(call, check=True)
    same(a, b, list(shapes))
    want = frame_call(p, path, diag, view_bias=p['bias'])
    for n in shapes:
        eq(a, n, want[n])

    def short(k):
        assert call(k, ws_bytes=need - 1) == -4
    def orphan(k):
        assert call(k, off_args=[p['off'][0].data_ptr(), 16, p['off'][1].data_ptr(), p['off'][2].data_ptr()],
                    grid_args=[None, 0, None, None]) == -1
    for fn in (short, orphan):
        x, y = both(fn)
        for k in (x, y):
            for n in shapes:
                k.g[n].holds_fill()


# ================================================================================================ 7. datasets on the device
def test_device_routes_put_the_camera_directions_in_the_third_row(golden_dir):
    """With view_dir and view_dir_camera_only the device routes -- render.with_rays over ops.gen_rays for a camera-only
    movement frame, and DeviceFrameCache.train_batch -- return the host route's third row (the directions under the
    extrinsics before apply_global_tfm_to_camera, same ray selection) to the ray generator's 2e-6; without the options
    the third row stays a copy of row 1."""
    from humannerf_amd import dataset, render
    from humannerf_amd.config import cfg
    subj = dataset.Subject(os.path.join(golden_dir, 'subject_synth'))
    idx = 1                                                        # (Rh != 0 on this frame)
    H, W = subj.image_size(subj.framelist[idx])
    plain = render.with_rays(subj.movement_frame(idx, image_size=(H, W)), dev())
    assert torch.equal(plain['rays'][2], plain['rays'][1])
    old = (cfg.patch.N_patches, cfg.patch.size)
    cfg.patch.N_patches, cfg.patch.size = 4, 16
    try:
        with vc.view_config(camera_only=True):
            want = subj.movement_frame(idx, host_rays=True, image_size=(H, W))
            got = render.with_rays(subj.movement_frame(idx, image_size=(H, W)), dev())
            assert got['rays'].shape == want['rays'].shape
            np.testing.assert_allclose(got['rays'].cpu().numpy(), want['rays'], rtol=2e-6, atol=2e-6)
            assert np.abs(want['rays'][2] - want['rays'][1]).max() > 1e-3
            cache = dataset.DeviceFrameCache(subj, dev())
            np.random.seed(5)
            item_want = subj.train_frame(idx)
            np.random.seed(5)
            item = cache.train_batch(idx)
            np.testing.assert_allclose(item['rays'].cpu().numpy(), item_want['rays'], rtol=2e-6, atol=2e-6)
            assert np.abs(item_want['rays'][2] - item_want['rays'][1]).max() > 1e-3
        np.random.seed(5)
        item = cache.train_batch(idx)                              # the options off again: the same entry, [o, d, d]
        assert torch.equal(item['rays'][2], item['rays'][1])
    finally:
        cfg.patch.N_patches, cfg.patch.size = old
