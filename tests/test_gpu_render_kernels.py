"""The kernels around the MLPs on the render path -- K1 sampling and warp, compaction, ray generation, K4 compositing,
the slab-wise termination path, the sparse MLP launches -- against fp64, instance by instance (DESIGN.md section 2 has
the table of instances and the test that checks each one's values).

References and problem builders: tests/test_render_kernel_refs.py (plain torch / numpy on the CPU, checked there
without a GPU).  Tolerances: 4 x the error of the reference's own fp32 evaluation against its fp64 evaluation on the
same inputs (at least 2e-7 of the quantity's scale), computed here; where an older test states a tolerance for the same
quantity, the smaller of the two.  Every test prints its ratio of kernel error to that floor (``pytest -s``;
profiles/render_kernel_tests.txt has the values of one run)."""

import numpy as np
import pytest
import torch

from tests import test_render_kernel_refs as refs

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(name, got, ref64, ref32, sel=None, cap=None):
    """max |got - ref64| <= 4 x floor (refs.tolerance), optionally capped by an older test's tolerance."""
    tol, floor = refs.tolerance(ref32, ref64, sel)
    g, r = torch.as_tensor(got).double().reshape(ref64.shape), ref64.double()
    if sel is not None:
        g, r = g[sel], r[sel]
    err = float((g - r).abs().max()) if r.numel() else 0.0
    if cap is not None:
        tol = min(tol, cap)
    print('RATIO %s err %.3e floor %.3e ratio %.2f' % (name, err, floor, err / floor if floor else 0.0))
    assert bool(torch.isfinite(g).all()), name
    assert err <= tol, (name, err, tol, floor)


# ------------------------------------------------------------------------------------------------ 1. K1 vs fp64
def _k1(pr, use_t_rand, want_bmw):
    from humannerf_amd import ops
    out = ops.sample_warp(T(pr['rays_o']), T(pr['rays_d']), T(pr['near']), T(pr['far']),
                          T(pr['t_rand']) if use_t_rand else None, T(pr['Rs']), T(pr['Ts']), T(pr['vol']), T(pr['bmin']),
                          T(pr['bscale']), pr['S'], want_bmw=want_bmw)
    torch.cuda.synchronize()
    return [None if o is None else o.cpu() for o in out]


@pytest.mark.parametrize('use_t_rand', [False, True])
@pytest.mark.parametrize('case', refs.K1_CASES, ids=lambda c: 'B%d_G%d_S%d_R%d_x%d' % c)
def test_k1_against_fp64(case, use_t_rand):
    """All four instances of sample_warp_kernel (bone count 24 at compile time / read at run time, with / without the
    per-bone weight output) at every shape of refs.K1_CASES: z, per-bone weights, weight sum, the numerator x_skel *
    max(sum w, 1e-4) on EVERY sample (it has no conditioning problem), and x_skel itself where sum w >= 1e-2."""
    B, G, S, R, _ = case
    pr = refs.k1_problem(*case)
    r64, r32 = refs.ref_k1(pr, use_t_rand), refs.ref_k1(pr, use_t_rand, torch.float32)
    z, xs, m, bmw = _k1(pr, use_t_rand, True)
    tag = 'k1 B%d G%d S%d R%d t%d ' % (B, G, S, R, use_t_rand)
    _check(tag + 'z', z, r64['z'], r32['z'], cap=1e-6)
    _check(tag + 'w', bmw.reshape(-1, B), r64['w'], r32['w'], cap=2e-5)
    _check(tag + 'wsum', m.reshape(-1), r64['wsum'], r32['wsum'], cap=1e-4)
    num = xs.reshape(-1, 3).double() * m.reshape(-1).double().clamp(min=0.0001)[:, None]
    fin = r64['num'].abs().amax(1) < 1e3                     # (the ray placed 1e6 away: its weights are 0, checked above)
    assert bool((m.reshape(-1)[~fin] == 0).all()) and bool((xs.reshape(-1, 3)[~fin] == 0).all())
    _check(tag + 'num', num, r64['num'], r32['num'], sel=fin[:, None].expand(-1, 3))
    ok = r64['wsum'] >= 1e-2
    assert float(ok.double().mean()) >= 0.70
    _check(tag + 'x_skel', xs.reshape(-1, 3), r64['x'], r32['x'], sel=ok[:, None].expand(-1, 3), cap=2e-4)
    # the lean instance: the same bits
    z2, xs2, m2, none = _k1(pr, use_t_rand, False)
    assert none is None and torch.equal(z, z2) and torch.equal(xs, xs2) and torch.equal(m, m2)


@pytest.mark.parametrize('case', [refs.K1_CASES[4], refs.K1_CASES[6], refs.K1_CASES[8]], ids=lambda c: 'B%d_G%d_S%d_R%d_x%d' % c)
def test_k1_inside_the_clamp_of_the_weight_sum(case):
    """Planted: the whole volume scaled by 2e-6, so that 0 < sum w < 1e-4 wherever a sample meets the lattice and x_skel
    = numerator / 1e-4: the clamp decides the value, and x_skel is compared on every sample."""
    B = case[0]
    pr = refs.k1_problem(*case, vol_scale=2e-6)
    r64, r32 = refs.ref_k1(pr, False), refs.ref_k1(pr, False, torch.float32)
    assert float(r64['wsum'].max()) < 1e-4 and float((r64['wsum'] > 0).double().mean()) > 0.5
    z, xs, m, bmw = _k1(pr, False, True)
    tag = 'k1-clamp B%d G%d ' % (B, case[1])
    _check(tag + 'w', bmw.reshape(-1, B), r64['w'], r32['w'])
    _check(tag + 'wsum', m.reshape(-1), r64['wsum'], r32['wsum'])
    _check(tag + 'x_skel', xs.reshape(-1, 3), r64['x'], r32['x'])


# ------------------------------------------------------------------------------------------------ 2. K1 exact cases
@pytest.mark.parametrize('B', [24, 7])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_k1_exact_lattice_cases(axis, B):
    """refs.k1_exact_problem: every sample is a lattice node or the midpoint of 2 / 4 / 8 nodes, in exact fp32
    arithmetic (1 / 32 and its multiples: z is exact whatever the division instruction does, asserted).  The per-bone
    weight must equal the stored entry, or the exact average, BIT FOR BIT: on nodes of the faces (x0 = G - 1: the pair
    gather's second element with weight 1), half a cell outside (x0 = -1 or G - 1: the in-range neighbour with weight
    1/2) and a whole cell outside (exactly 0).  Both the staged (B = 24) and the plain (B = 7) weight output."""
    pr, lat = refs.k1_exact_problem(axis, B)
    z, xs, m, bmw = _k1(pr, False, True)
    assert np.array_equal(z.numpy(), np.tile(np.arange(33, dtype=np.float32) / 16, (pr['R'], 1)))
    want = refs.exact_lattice_weights(pr['vol'][:B], lat)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    got = bmw.numpy().astype(np.float64)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), lat[tuple(bad[0][:2])].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(m.numpy().astype(np.float64), want.sum(-1))        # (multiples of 2^-13: the sum is exact too)
    outside = ((lat < 0) | (lat > 32)).any(-1) & (lat == np.floor(lat)).all(-1)
    assert outside.any() and (got[outside] == 0).all()


@pytest.mark.parametrize('S', refs.K1_Z_EXACT_S)
def test_k1_z_equals_its_fp32_statement_bit_for_bit(S):
    """z against refs.z_statement_fp32 (the reference's expressions in numpy fp32, one rounding per operation, linspace's
    element in its two forms), bit for bit, with and without the stratified jitter.  At these S the two forms differ by
    an ulp at the midpoint S // 2 (tests/test_render_kernel_refs.py): taking the wrong one there is invisible to any
    tolerance against fp64.  Measured: K1 equals the statement on every element; torch.linspace on the device does not
    (an ulp on 1 of 16 to 23 of 256 elements), so the bit-for-bit claim is about these forms, not about torch's kernel."""
    pr = refs.k1_problem(3, 4, S, 9)
    pr['near'][1], pr['far'][1] = 0.0, 1.0                      # z = t itself
    for tr in (None, pr['t_rand']):
        z = _k1(pr, tr is not None, False)[0].numpy()
        want = refs.z_statement_fp32(pr['near'], pr['far'], S, tr)
        assert np.array_equal(z, want), (S, tr is not None, int((z != want).sum()))
        if tr is None:
            assert z[1, S // 2] == refs.linspace_midpoint_forms(S)[1]


# ------------------------------------------------------------------------------------------------ 3. K1 argument checks
def test_k1_refuses_before_launching():
    """S = 1, G = 1, B = 0 and a per-bone weight pointer off 16-byte alignment with 24 bones return HNRF_E_ARG; the same
    pointer with 7 bones is accepted; R = 0 returns without touching the outputs."""
    from humannerf_amd import _lib
    lib = _lib.load()
    pr = refs.k1_problem(24, 8, 4, 5)
    a = {k: T(pr[k]) for k in ('rays_o', 'rays_d', 'near', 'far', 'Rs', 'Ts', 'vol', 'bmin', 'bscale')}
    R, S = 5, 4
    z, xs, m = (torch.full((R * S * n,), -7.0, device=dev()) for n in (1, 3, 1))
    bmw = torch.full((R * S * 24 + 4,), -7.0, device=dev())
    assert bmw.data_ptr() % 16 == 0

    def call(R_, S_, B_, G_, bmw_ptr):
        return lib.hnrf_sample_warp_fwd(a['rays_o'].data_ptr(), a['rays_d'].data_ptr(), a['near'].data_ptr(),
                                        a['far'].data_ptr(), None, a['Rs'].data_ptr(), a['Ts'].data_ptr(),
                                        a['vol'].data_ptr(), a['bmin'].data_ptr(), a['bscale'].data_ptr(), R_, S_, B_, G_,
                                        z.data_ptr(), xs.data_ptr(), m.data_ptr(), bmw_ptr, _stream())
    E_ARG = -1                                           # HNRF_E_ARG
    assert call(R, 1, 24, 8, None) == E_ARG
    assert call(R, S, 24, 1, None) == E_ARG
    assert call(R, S, 0, 8, None) == E_ARG
    assert call(R, S, 24, 8, bmw.data_ptr() + 4) == E_ARG
    assert b'16-byte' in lib.hnrf_last_error()
    assert call(0, S, 24, 8, bmw.data_ptr()) == 0
    torch.cuda.synchronize()
    for t in (z, xs, m, bmw):
        assert bool((t == -7.0).all())
    assert call(R, S, 7, 8, bmw.data_ptr() + 4) == 0
    torch.cuda.synchronize()
    assert bool((bmw[1:1 + R * S * 7] != -7.0).all()) and bool((bmw[1 + R * S * 7:] == -7.0).all()) and float(bmw[0]) == -7.0
    assert call(R, S, 24, 8, bmw.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((bmw[:R * S * 24] != -7.0).all()) and bool((bmw[R * S * 24:] == -7.0).all())
    assert bool((z != -7.0).all())


# ------------------------------------------------------------------------------------------------ 4. ray generation
@pytest.mark.parametrize('name', list(refs.RAYGEN_CAMERAS))
def test_ray_generation_on_oblique_cameras(name):
    """hnrf_gen_rays on cameras off every axis, off centre, inside the box and on tiny images (uneven block counts; more
    than 1024 blocks: several per thread of the scan).  The mask equals the reference's except on grazing rays (margin <
    1e-5, at most 0.2 % of the pixels: asserted from the reference); rays / near / far are scattered back through the
    DEVICE mask and compared at every pixel both keep -- a wrong block offset or rank moves them to other pixels."""
    from humannerf_amd import ops
    r = refs.ref_raygen(name)
    H, W = r['H'], r['W']
    graze = r['margin'] < refs.RAYGEN_MARGIN
    assert graze.mean() <= refs.RAYGEN_MAX_GRAZING
    got = ops.gen_rays(r['K'], r['E'], r['mn'], r['mx'], H, W)
    gm = got['ray_mask'].cpu().numpy()
    assert gm.shape == r['hit'].shape
    diff = gm != r['hit']
    print('RATIO raygen %s pixels %d kept %d grazing %d (%.4f %%) mask differs on %d' %
          (name, H * W, r['hit'].sum(), graze.sum(), 100.0 * graze.mean(), diff.sum()))
    assert not (diff & ~graze).any(), int((diff & ~graze).sum())
    n = int(gm.sum())
    assert got['rays'].shape == (3, n, 3) and got['near'].shape == (n, 1) and got['far'].shape == (n, 1)   # count
    assert torch.equal(got['rays'][1], got['rays'][2])
    both = gm & r['hit']
    full = np.full((H * W, 8), np.nan, np.float32)
    full[gm] = np.concatenate([got['rays'][0].cpu().numpy(), got['rays'][1].cpu().numpy(), got['near'].cpu().numpy(),
                               got['far'].cpu().numpy()], 1)
    want = np.full((H * W, 8), np.nan, np.float32)
    want[r['hit']] = np.concatenate([r['ro'][r['hit']], r['rd'][r['hit']], r['near'][:, None], r['far'][:, None]], 1)
    np.testing.assert_allclose(full[both, :3], want[both, :3], rtol=0, atol=1e-6)
    np.testing.assert_allclose(full[both, 3:], want[both, 3:], rtol=2e-6, atol=2e-6)
    if both.any():
        print('RATIO raygen %s max err o %.2e d %.2e near/far %.2e' % (
            name, np.abs(full[both, :3] - want[both, :3]).max(), np.abs(full[both, 3:6] - want[both, 3:6]).max(),
            np.abs(full[both, 6:] - want[both, 6:]).max()))


# ------------------------------------------------------------------------------------------------ 5. compaction, sparse MLPs
def _compact(mask_np, eps):
    """hnrf_compact_samples through the C ABI into an idx pre-filled with -1 (one spare element in front of and behind
    the P the kernel is told about) -> (idx, count)."""
    from humannerf_amd import _lib
    lib = _lib.load()
    P = len(mask_np)
    m = T(np.concatenate([mask_np, np.ones(1, np.float32)]).astype(np.float32))
    idx = torch.full((P + 2,), -1, dtype=torch.int32, device=dev())
    count = torch.full((1,), -5, dtype=torch.int32, device=dev())
    _lib.check(lib.hnrf_compact_samples(m.data_ptr(), float(eps), P, idx.data_ptr() + 4, count.data_ptr(), _stream()),
               'hnrf_compact_samples')
    torch.cuda.synchronize()
    assert int(idx[0]) == -1 and int(idx[-1]) == -1
    return idx[1:1 + P].cpu().numpy(), int(count.item())


def _empty_block_mask():
    """769 samples of which eps = 0.5 keeps all of block 0, none of block 1 (it issues no atomic), three scattered ones of
    block 2 and the one sample of block 3."""
    m = np.zeros(769, np.float32)
    m[:256] = 1
    m[[512 + 5, 512 + 64, 512 + 255, 768]] = 1
    return m


COMPACT_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 100003]


@pytest.mark.parametrize('P,mask', [(P, None) for P in COMPACT_SIZES] + [(769, _empty_block_mask())],
                         ids=[str(P) for P in COMPACT_SIZES] + ['empty-block'])
def test_compaction_sets_counts_and_bounds(P, mask):
    """Exact index set and count; nothing written at or past idx[count]; a NaN entry is never kept.  mask None: random
    values with every seventh zero."""
    if mask is not None:
        m = mask.copy()
    else:
        rs = np.random.RandomState(P)
        m = rs.uniform(0, 1, P).astype(np.float32)
        m[::7] = 0
    if P:
        m[P // 2] = np.nan
    nan = np.isnan(m)
    for eps, keep in ((0.5, ~nan & (m >= 0.5)), (0.0, ~nan), (2.0, np.zeros(P, bool)), (1e-30, ~nan & (m > 0))):
        idx, n = _compact(m, eps)
        assert n == int(keep.sum()), (eps, n)
        assert np.array_equal(np.sort(idx[:n]), np.nonzero(keep)[0])
        assert (idx[n:] == -1).all()
    idx, n = _compact(np.ones(P, np.float32), 1.0)                           # keeps everything
    assert n == P and np.array_equal(np.sort(idx), np.arange(P))


SPARSE_COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]


@pytest.fixture(scope='module')
def sparse_setup():
    """Packed weights and dense results of K2 and K3 on 300 positions, per mode; the positions / outputs sit inside
    larger buffers (8 rows of margin on both sides)."""
    from humannerf_amd import ops
    from tests.test_train_kernel_refs import make_problem
    P, M = 300, 8
    out = {}
    for kind in ('canonical', 'nonrigid'):
        pr = make_problem(kind, P, 77, 'scaled' if kind == 'nonrigid' else None)
        xbuf = torch.zeros(P + 2 * M, 3, device=dev())
        xbuf[M:M + P] = T(pr['x'])
        for mode in ('f32', 'f16x3'):
            ws, bs = [T(w) for w in pr['ws']], [T(b) for b in pr['bs']]
            if kind == 'canonical':
                packed = ops.canonical_pack(ws, bs, mode)
                dense = ops.canonical(xbuf[M:M + P], packed, mode)
                hann = None
            else:
                packed = ops.nonrigid_pack(ws, bs, T(pr['cond']), mode)
                hann = T(pr['hann'])
                dense, _ = ops.nonrigid(xbuf[M:M + P], hann, packed, mode)
            out[kind, mode] = dict(P=P, M=M, xbuf=xbuf, packed=packed, dense=dense, hann=hann)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
@pytest.mark.parametrize('kind', ['canonical', 'nonrigid'])
def test_sparse_mlp_launches_equal_dense_on_the_listed_samples(kind, mode, sparse_setup):
    """hnrf_canonical_fwd_sparse / hnrf_nonrigid_fwd_sparse on a shuffled subset of 300 samples, count at the wave and
    workgroup edges: the listed rows equal the dense launch bit for bit, every other row of the sentinel-filled output
    (margins included) is unchanged, the idx entries past count hold -1 (reading one would show as a changed margin
    row), and the count is read on the device."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    s = sparse_setup[kind, mode]
    P, M = s['P'], s['M']
    C = 4 if kind == 'canonical' else 3
    rs = np.random.RandomState(3)
    for n in SPARSE_COUNTS:
        perm = rs.permutation(P)[:n]
        idx_h = np.full(P, -1, np.int32)
        idx_h[:n] = perm
        idx, count = T(idx_h), torch.tensor([n], dtype=torch.int32, device=dev())
        obuf = torch.full((P + 2 * M, C), 12345.0, device=dev())
        x, o = s['xbuf'][M:M + P], obuf[M:M + P]
        assert o.data_ptr() % 16 == 0
        if kind == 'canonical':
            rc = lib.hnrf_canonical_fwd_sparse(x.data_ptr(), s['packed'].data_ptr(), ops._mode_arg(mode), P, idx.data_ptr(),
                                               count.data_ptr(), o.data_ptr(), _stream())
        else:
            rc = lib.hnrf_nonrigid_fwd_sparse(x.data_ptr(), s['hann'].data_ptr(), s['packed'].data_ptr(), ops._mode_arg(mode),
                                              P, idx.data_ptr(), count.data_ptr(), o.data_ptr(), None, _stream())
        _lib.check(rc, 'sparse ' + kind)
        torch.cuda.synchronize()
        listed = torch.zeros(P + 2 * M, dtype=torch.bool, device=dev())
        listed[M + torch.from_numpy(perm).to(dev())] = True
        assert torch.equal(obuf[listed], s['dense'].reshape(P, C)[listed[M:M + P]]), (kind, mode, n)
        assert bool((obuf[~listed] == 12345.0).all()), (kind, mode, n)
        assert int(count.item()) == n and torch.equal(idx.cpu(), torch.from_numpy(idx_h))


# ------------------------------------------------------------------------------------------------ 6. K4
_K4_KEYS = ('rgb', 'alpha', 'depth', 'weights_on_rays', 'rgb_on_rays', 'cnl_weight', 'cnl_rgb')


def _k4(c, cull_eps=0.0):
    from humannerf_amd import ops
    out = ops.composite(T(c['raw']), T(c['mask']), T(c['z']), T(c['rays_d']), T(c['xyz']), T(c['bg']), diagnostics=True,
                        cull_eps=cull_eps)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _k4_compare(tag, c, out, cull_eps=0.0):
    r64, r32 = refs.ref_k4(c, cull_eps=cull_eps), refs.ref_k4(c, torch.float32, cull_eps=cull_eps)
    live = torch.from_numpy(c['mask'] >= cull_eps) if cull_eps > 0 else None
    w = np.sort(r64['weights_on_rays'].numpy(), axis=1)
    clear = torch.from_numpy((w[:, -1] - w[:, -2]) > 1e-6)                 # unambiguous argmax
    assert float(clear.double().mean()) >= 0.9
    for k in _K4_KEYS:
        sel = None
        if k == 'rgb_on_rays' and live is not None:
            sel = live[..., None].expand(-1, -1, 3)                        # culled samples: raw is undefined, the kernel writes 0
            assert bool((out[k][~sel] == 0).all())
        if k == 'cnl_rgb':
            sel = clear[:, None].expand(-1, 3)
        _check(tag + k, out[k], r64[k], r32[k], sel=sel, cap=3e-6 * max(1.0, float(r64[k].abs().max())))
    assert torch.equal(out['cnl_xyz'][clear], r64['cnl_xyz'][clear].float())


@pytest.mark.parametrize('regime', ['sparse', 'dense', 'opaque'])
@pytest.mark.parametrize('S,R', list(zip(refs.K4_S, refs.K4_R)))
def test_k4_across_instances(S, R, regime):
    """composite_kernel<1|2|4|8> at the edges of every instance (S in (128, 192] rounds 3 samples per lane up to 4 and
    leaves whole trailing lanes empty), ray counts 1..5 and ragged, all eight outputs, in the three regimes of
    composite_problem."""
    c = refs.k4_problem(R, S, regime)
    _k4_compare('k4 %s S%d R%d ' % (regime, S, R), c, _k4(c))


@pytest.mark.parametrize('S,R', [(3, 5), (65, 4), (150, 37), (192, 1), (257, 4), (512, 37)])
def test_k4_culled_samples_with_undefined_raw(S, R):
    """cull_eps > 0: raw at every sample with mask < cull_eps is NaN (such samples never went through the MLPs).  All
    outputs are finite and equal the reference with those samples at alpha = 0."""
    c = refs.k4_problem(R, S, 'sparse')
    culled = c['mask'] < refs.K4_CULL_EPS
    assert 0.1 < culled.mean() < 0.5
    c['raw'] = np.where(culled[..., None], np.float32(np.nan), c['raw'])
    out = _k4(c, refs.K4_CULL_EPS)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    _k4_compare('k4-cull S%d R%d ' % (S, R), c, out, refs.K4_CULL_EPS)


@pytest.mark.parametrize('S', [2, 65, 150, 192, 512])
def test_k4_exact_ties_gather_the_first(S):
    """refs.k4_tie_problem: an all-zero-weight ray gathers sample 0; of two equal largest weights the first is gathered
    (what the oracle's max returns in fp32: tests/test_render_kernel_refs.py)."""
    c, firsts = refs.k4_tie_problem(S)
    out = _k4(c)
    w = out['weights_on_rays'].numpy()
    assert (w[0] == 0).all() and float(out['cnl_weight'][0]) == 0.0
    want = [0, firsts[1], firsts[2]]
    for r in (1, 2):
        assert w[r, firsts[r]] == w[r, S - 1] == np.float32(0.5) and float(out['cnl_weight'][r]) == 0.5
    assert np.array_equal(out['cnl_xyz'].numpy(), c['xyz'][np.arange(3), want])
    assert torch.equal(out['cnl_rgb'], out['rgb_on_rays'][torch.arange(3), torch.tensor(want)])


def test_k4_refuses_more_than_512_samples():
    from humannerf_amd import _lib
    c = refs.k4_problem(2, 513, 'sparse')
    with pytest.raises(_lib.HnrfError, match='513'):
        _k4(c)


# ------------------------------------------------------------------------------------------------ 7. termination path
@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
@pytest.mark.parametrize('case', refs.TERM_CASES, ids=lambda c: 'S%d_R%d_nr%d_t%d_cull%g_term%g_bias%g' % c)
def test_termination_path_against_the_slab_walk(case, mode):
    """hnrf_render_rays_term_fwd against refs.ref_slab_walk in fp64.  The walk is fed the dense raw of the same kernels
    in the same mode (ops.sample_warp -> ops.nonrigid -> ops.canonical), so only the slab logic is under test: which
    samples are evaluated, the running transmittance across slabs (ragged last slab, ragged last workgroup), the
    culling of both kinds together.  Rays whose transmittance at a slab entry lies within relative 1e-4 of term_eps are
    ambiguous (at most 1 % of a case); rgb / alpha / depth are compared on the others, and the evaluated-sample count
    lies between the reference's with the ambiguous rays all dead and all alive."""
    from humannerf_amd import ops
    S, R, with_nr, use_t, cull_eps, term_eps, bias = case
    pr = refs.term_problem(R, S, bias)
    g = {k: T(pr[k]) for k in ('rays_o', 'rays_d', 'near', 'far', 'Rs', 'Ts', 'vol', 'bmin', 'bscale', 'hann', 'bg')}
    t_rand = T(pr['t_rand']) if use_t else None
    cnp = ops.canonical_pack([T(w) for w in pr['cw']], [T(b) for b in pr['cb']], mode)
    nrp = ops.nonrigid_pack([T(w) for w in pr['nw']], [T(b) for b in pr['nb']], T(pr['cond']), mode) if with_nr else None
    hann = g['hann'] if with_nr else None
    args = (g['rays_o'], g['rays_d'], g['near'], g['far'], t_rand, g['Rs'], g['Ts'], g['vol'], g['bmin'], g['bscale'])
    z, xs, mask, _ = ops.sample_warp(*args, S)
    xyz = ops.nonrigid(xs, hann, nrp, mode)[0] if with_nr else xs
    raw = ops.canonical(xyz, cnp, mode)
    out = ops.render_rays_term(*args, hann, nrp, cnp, g['bg'], S, mode, term_eps=term_eps, cull_eps=cull_eps,
                               want_count=True)
    torch.cuda.synchronize()
    walk = lambda dt, amb=None: refs.ref_slab_walk(raw.cpu().to(dt), mask.cpu().to(dt), z.cpu().to(dt),
                                                   g['rays_d'].cpu().to(dt), g['bg'].cpu().to(dt), cull_eps, term_eps,
                                                   ambiguous=amb)
    r64, r32 = walk(torch.float64), walk(torch.float32)
    clear = r64['closeness'] >= refs.TERM_BAND
    share = 1.0 - float(clear.double().mean())
    n = int(out['evaluated'].item())
    lo, hi = walk(torch.float64, False)['evaluated'], walk(torch.float64, True)['evaluated']
    print('RATIO term %s S%d R%d nr%d t%d cull%g term%g bias%g ambiguous %.4f evaluated %d of %d (reference %d..%d)' %
          (mode, S, R, with_nr, use_t, cull_eps, term_eps, bias, share, n, R * S, lo, hi))
    assert share <= refs.TERM_MAX_AMBIGUOUS
    tag = 'term %s S%d R%d bias%g ' % (mode, S, R, bias)
    for k in ('rgb', 'alpha', 'depth'):
        sel = clear[:, None].expand(-1, 3) if k == 'rgb' else clear
        _check(tag + k, out[k].cpu(), r64[k], r32[k], sel=sel)
    assert lo <= n <= hi, (lo, n, hi)
    if share == 0.0:
        assert lo == hi == r64['evaluated'] == n


def test_termination_cases_saturate_in_every_slab():
    """The density biases of refs.TERM_CASES do what they are there for (from the kernels' own dense raw, in fp64): at S
    = 128 the rays of bias 80 are below 1e-2 before the second slab, those of bias 6 get there in the second to fourth
    slab or not at all, and at bias 2.5 most rays reach the last slab above it."""
    from humannerf_amd import ops
    died = {}
    for bias in (80.0, 6.0, 2.5):
        pr = refs.term_problem(64, 128, bias)
        g = {k: T(pr[k]) for k in ('rays_o', 'rays_d', 'near', 'far', 'Rs', 'Ts', 'vol', 'bmin', 'bscale', 'bg')}
        cnp = ops.canonical_pack([T(w) for w in pr['cw']], [T(b) for b in pr['cb']], 'f32')
        z, xs, mask, _ = ops.sample_warp(g['rays_o'], g['rays_d'], g['near'], g['far'], None, g['Rs'], g['Ts'], g['vol'],
                                         g['bmin'], g['bscale'], 128)
        raw = ops.canonical(xs, cnp, 'f32')
        o = refs.ref_k4(dict(raw=raw.cpu().numpy(), mask=mask.cpu().numpy(), z=z.cpu().numpy(), rays_d=pr['rays_d'],
                             xyz=xs.cpu().numpy(), bg=pr['bg']))
        Tr = 1.0 - torch.cumsum(o['weights_on_rays'], 1)                    # transmittance behind each sample
        died[bias] = [float((Tr[:, s] < 1e-2).double().mean()) for s in (31, 63, 95)]
    print('RATIO term share of rays under 1e-2 after slab 1 / 2 / 3:', died)
    assert died[80.0][0] > 0.9
    assert died[6.0][0] < 0.1 < died[6.0][1] < died[6.0][2] < 0.9
    assert died[2.5][2] < 0.5
