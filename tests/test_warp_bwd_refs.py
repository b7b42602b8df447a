"""fp64 reference, problem builders and case table of the sample-warp backward kernel K1' (tests/test_gpu_warp_bwd.py),
and the checks of them that need no GPU.  The reference is torch.autograd through oracle.sample_motion_fields on the CPU;
``dtype`` selects fp64 (the reference) or fp32 (the same expressions in the kernel's precision: its distance from fp64 is
the noise floor the tolerances are scaled by, tests/test_render_kernel_refs.py::tolerance).

The spatial derivative of a trilinear lookup jumps at the voxel faces, so a sample whose fp32 position lies on the other
side of a face than its fp64 position flips a whole term of d_Rs / d_Ts, in the kernel and in the reference's own fp32
evaluation alike.  ``face_filter`` names those samples from the fp64 positions alone and the problems carry a zero
incoming gradient for them (they are still processed, and still take part in the kernel's run folding): what is left is
smooth, and the fp32 floor drops from 1e-2 to about 2e-6 of the largest entry."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import test_render_kernel_refs as refs

FACE_DELTA, MASK_DELTA, MAX_ZEROED = 1e-4, 1e-6, 0.05
LDS_MIN_SAMPLES, LDS_MAX_G = 65536, 33          # the launcher's switch: LDS gradient grid from 65536 samples on, G <= 33


# ------------------------------------------------------------------------------------------------ problems
def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _points(pr, dtype=torch.float64):
    """pts = rays_o + rays_d * z from the fp32 z of the problem, (P, 3) in ``dtype``."""
    z = _t(pr['z'], dtype)
    return (_t(pr['rays_o'], dtype)[:, None] + _t(pr['rays_d'], dtype)[:, None] * z[:, :, None]).reshape(-1, 3)


def face_filter(pr, delta=FACE_DELTA, mask64=None):
    """Boolean (P,): samples that for some bone and axis lie within ``delta`` (in cells) of one of the faces -1, 0 .. G of
    the lattice, where the derivative of the zero-padded trilinear weight jumps, or whose weight sum lies within
    MASK_DELTA of the 1e-4 clamp.  From fp64 positions only.  Beyond the faces -1 and G nothing is selected: the weight
    and its derivative are identically zero there."""
    G = pr['G']
    pts = _points(pr)
    Rs, Ts, bmin, bscale = _t(pr['Rs']), _t(pr['Ts']), _t(pr['bmin']), _t(pr['bscale'])
    sel = torch.zeros(pts.shape[0], dtype=torch.bool)
    for b in range(pr['B']):
        c = ((pts @ Rs[b].T + Ts[b]) - bmin) * bscale * 0.5 * (G - 1)
        near_face = ((c - torch.round(c)).abs() < delta) & (c > -1 - delta) & (c < G + delta)
        sel |= near_face.any(-1)
    if mask64 is not None:
        sel |= (mask64 - 1e-4).abs() < MASK_DELTA
    return sel.numpy()


def k1_bwd_problem(case, seed=1, vol_scale=1.0, span=None, zero_dirs=False, rays=None, z=None, x_skel=None, fg_mask=None,
                   filtered=True, base=None, delta=FACE_DELTA):
    """Inputs of hnrf_sample_warp_bwd (numpy fp32) on the geometry refs.k1_problem(*case): z = oracle.z_values in fp64
    (stratified with the problem's t_rand), rounded; x_skel and fg_mask = the fp64 forward at rays_o + rays_d * z,
    rounded; incoming gradients g_x (P, 3), g_mask (P,) standard normal, zero on the samples of face_filter
    (``zeroed``).  span: far = near + span (a ray stays in one cell for tens of samples); zero_dirs: every rays_d = 0;
    rays: slice of the rays kept (of the geometry AND of the gradients: the parts of a problem add up to the whole);
    z, x_skel, fg_mask: given (a forward kernel's outputs) instead of computed; base: a ready geometry instead of
    refs.k1_problem; delta: of face_filter."""
    B, G, S, R, extra = case
    pr = dict(base) if base is not None else refs.k1_problem(B, G, S, R, extra, seed=seed, vol_scale=vol_scale)
    if span is not None:
        pr['far'] = (pr['near'] + np.float32(span)).astype(np.float32)
    if zero_dirs:
        pr['rays_d'] = np.zeros_like(pr['rays_d'])
    if z is None:
        tr = pr['t_rand']
        z = oracle.z_values(_t(pr['near']), _t(pr['far']), S, None if tr is None else _t(tr)).numpy()
    pr['z'] = np.ascontiguousarray(z, dtype=np.float32).reshape(R, S)
    rs = np.random.RandomState(1000 + seed + B + G + S + R)
    pr['g_x'] = rs.standard_normal((R * S, 3)).astype(np.float32)
    pr['g_mask'] = rs.standard_normal(R * S).astype(np.float32)
    if rays is not None:
        for k in ('rays_o', 'rays_d', 'near', 'far', 'z'):
            pr[k] = np.ascontiguousarray(pr[k][rays])
        for k in ('g_x', 'g_mask'):
            pr[k] = np.ascontiguousarray(pr[k].reshape((R, S) + pr[k].shape[1:])[rays]).reshape((-1,) + pr[k].shape[1:])
        pr['R'] = R = pr['z'].shape[0]
    pr['extra'], pr['P'] = extra, R * S
    with torch.no_grad():
        x64, m64, _ = oracle.sample_motion_fields(_points(pr), _t(pr['Rs']), _t(pr['Ts']), _t(pr['vol'])[:B + 1],
                                                  _t(pr['bmin']), _t(pr['bscale']))
    pr['x_skel'] = x64.float().numpy() if x_skel is None else np.ascontiguousarray(x_skel, np.float32).reshape(-1, 3)
    pr['fg_mask'] = m64.float().numpy() if fg_mask is None else np.ascontiguousarray(fg_mask, np.float32).reshape(-1)
    pr['mask64'] = m64.numpy()
    pr['zeroed'] = face_filter(pr, delta, m64) if filtered else np.zeros(R * S, bool)
    pr['g_x'][pr['zeroed']] = 0
    pr['g_mask'][pr['zeroed']] = 0
    return pr


def grad_suite_problem(R, G, S, span, filtered):
    """The problem of tests/test_gpu_grad.py::test_sample_warp_bwd_kernel (same generator, same order of draws), with
    z from the oracle instead of the forward kernel."""
    rs = np.random.RandomState(9)
    B = 24
    rays_o = rs.uniform(-0.3, 0.3, (R, 3)).astype(np.float32)
    rays_d = rs.uniform(-1, 1, (R, 3)).astype(np.float32)
    near = rs.uniform(0.0, 0.2, (R, 1)).astype(np.float32)
    far = near + rs.uniform(span, 2 * span, (R, 1)).astype(np.float32)
    Rs = (np.eye(3)[None] + 0.1 * rs.randn(B, 3, 3)).astype(np.float32)
    Ts = (0.1 * rs.randn(B, 3)).astype(np.float32)
    vol = rs.uniform(0, 0.1, (B + 1, G, G, G)).astype(np.float32)
    bmin = np.array([-1.0, -1.1, -0.9], dtype=np.float32)
    bscale = (2.0 / np.array([2.0, 2.2, 1.8])).astype(np.float32)
    base = dict(rays_o=rays_o, rays_d=rays_d, near=near, far=far, Rs=Rs, Ts=Ts, vol=vol, bmin=bmin, bscale=bscale,
                t_rand=None, B=B, G=G, S=S, R=R)
    pr = k1_bwd_problem((B, G, S, R, 1), base=base, filtered=False)
    pr['g_x'], pr['g_mask'] = rs.randn(R, S, 3).astype(np.float32).reshape(-1, 3), rs.randn(R, S).astype(np.float32).reshape(-1)
    if filtered:
        pr['zeroed'] = face_filter(pr, mask64=torch.from_numpy(pr['mask64']))
        pr['g_x'][pr['zeroed']] = 0
        pr['g_mask'][pr['zeroed']] = 0
    return pr


# ------------------------------------------------------------------------------------------------ reference
def ref_k1_bwd(pr, dtype=torch.float64):
    """torch.autograd through oracle.sample_motion_fields in ``dtype`` for the loss <x_skel, g_x> + <fg_mask, g_mask>, at
    pts = rays_o + rays_d * z with the fp32 z of the problem: dict(vol (B, G, G, G), Rs (B, 3, 3), Ts (B, 3)).  The loss
    is a sum over samples: it is walked in chunks of samples that bound the memory of the graph (one chunk up to
    65536 samples x 24 bones), the gradients of the chunks added in ``dtype``."""
    B, P = pr['B'], pr['P']
    pts = _points(pr, dtype)
    Rs, Ts = _t(pr['Rs'], dtype).requires_grad_(True), _t(pr['Ts'], dtype).requires_grad_(True)
    vol = _t(pr['vol'], dtype)[:B + 1].clone().requires_grad_(True)
    bmin, bscale = _t(pr['bmin'], dtype), _t(pr['bscale'], dtype)
    gx, gm = _t(pr['g_x'], dtype), _t(pr['g_mask'], dtype)
    chunk = max(1 << 14, (3 << 19) // B)
    for a in range(0, P, chunk):
        x, m, _ = oracle.sample_motion_fields(pts[a:a + chunk], Rs, Ts, vol, bmin, bscale)
        ((x * gx[a:a + chunk]).sum() + (m * gm[a:a + chunk]).sum()).backward()
    return dict(vol=vol.grad[:B].detach(), Rs=Rs.grad.detach(), Ts=Ts.grad.detach())


# ------------------------------------------------------------------------------------------------ fp32 twin
TWIN_FAULTS = ('drop_last_partial_wave', 'upper_cell', 'low_mask_term', 'clamped_corner', 'ts_last_block')


def k1_bwd_twin(pr, fault=None, f=np.float32):
    """The formulas of the kernel's header comment in numpy fp32, vectorised over samples, bone by bone:
         den = max(mask, 1e-4), gA = g_x / den, g_ws = g_mask - [mask >= 1e-4] (g_x . x_skel) / den
         dL/dw_b = gA . pos_b + g_ws
         corner weights: per axis (f0 + 1 - i, i - f0), zero for a corner outside the grid (addresses clamped)
         d_vol_b[corner] += dL/dw_b * corner weight
         d pos_b = w_b gA + dL/dw_b * grad_pos trilinear(vol_b);  d_Rs_b = sum d pos_b (x) pts, d_Ts_b = sum d pos_b
    ``fault``: one of TWIN_FAULTS, the planted mistakes a test of the kernel has to notice."""
    B, G, P = pr['B'], pr['G'], pr['P']
    z = pr['z'].reshape(-1, 1).astype(f)
    pts = (np.repeat(pr['rays_o'], pr['S'], 0) + np.repeat(pr['rays_d'], pr['S'], 0) * z).astype(f)
    m, xs, gx, gm = pr['fg_mask'], pr['x_skel'], pr['g_x'], pr['g_mask']
    live = np.ones(P, bool)
    if fault == 'drop_last_partial_wave':
        live[P - P % 64:] = False
    den = np.maximum(m, f(1e-4))
    gA = (gx / den[:, None]).astype(f)
    term = ((gx * xs).sum(1) / den).astype(f)
    gws = gm - (term if fault == 'low_mask_term' else np.where(m >= f(1e-4), term, f(0)))
    d_vol, d_Rs, d_Ts = np.zeros((B, G * G * G), f), np.zeros((B, 3, 3), f), np.zeros((B, 3), f)
    half = (pr['bscale'] * f(0.5) * f(G - 1)).astype(f)
    for b in range(B):
        q = (pts @ pr['Rs'][b].T + pr['Ts'][b]).astype(f)
        ic = ((q - pr['bmin']) * pr['bscale'] * f(0.5) * f(G - 1)).astype(f)
        f0 = np.floor(ic)
        if fault == 'upper_cell':
            f0[::200, 0] += 1
        i0 = np.clip(f0, -2, G + 1).astype(np.int64)
        wa, sa, ia = [], [], []                      # per corner offset 0 / 1: weight, its derivative, clamped index (P, 3)
        for o in (0, 1):
            ok = (i0 + o >= 0) & (i0 + o < G)
            if fault == 'clamped_corner':
                ok = np.ones_like(ok)
            wgt = (f0 + 1 - ic) if o == 0 else (ic - f0)
            wa.append(np.where(ok, wgt, 0).astype(f))
            sa.append(np.where(ok, f(2 * o - 1), f(0)))
            ia.append(np.clip(i0 + o, 0, G - 1))
        dLdw = ((gA * q).sum(1) + gws).astype(f) * live
        v = pr['vol'][b].reshape(-1)
        w, dw = np.zeros(P, f), np.zeros((P, 3), f)
        for oz in (0, 1):
            for oy in (0, 1):
                for ox in (0, 1):
                    idx = (ia[oz][:, 2] * G + ia[oy][:, 1]) * G + ia[ox][:, 0]
                    wx, wy, wz = wa[ox][:, 0], wa[oy][:, 1], wa[oz][:, 2]
                    vc = v[idx]
                    w += vc * wx * wy * wz
                    dw[:, 0] += vc * sa[ox][:, 0] * wy * wz
                    dw[:, 1] += vc * wx * sa[oy][:, 1] * wz
                    dw[:, 2] += vc * wx * wy * sa[oz][:, 2]
                    d_vol[b] += np.bincount(idx, weights=dLdw * (wx * wy * wz), minlength=G * G * G).astype(f)
        dq = ((w[:, None] * gA + dLdw[:, None] * dw * half) * live[:, None]).astype(f)
        dq64 = dq.astype(np.float64)                 # (the sums over samples in fp64: this states the terms, not their order)
        d_Rs[b] = dq64.T @ pts.astype(np.float64)
        d_Ts[b] = (dq64[:(P - 1) // 256 * 256] if fault == 'ts_last_block' and b == B - 1 else dq64).sum(0)
    return dict(vol=d_vol.reshape(B, G, G, G), Rs=d_Rs, Ts=d_Ts)


# ------------------------------------------------------------------------------------------------ cases
def _name(c):
    return 'B%d_G%d_S%d_R%d_x%d' % c


# name -> (case (B, G, S, R, extra), keyword arguments of k1_bwd_problem); seeds: SEEDS below.  The face filter zeroes at
# most 5 % of every case's samples (test_zeroed_share_is_capped).
GLOBAL_CASES = {_name(c): (c, {}) for c in refs.K1_CASES}
GLOBAL_CASES.update({'edge_P%d' % (R * S): ((3, 8, S, R, 1), {}) for R, S in
                     ((21, 3), (32, 2), (13, 5), (85, 3), (128, 2), (1, 257), (1, 2))})
GLOBAL_CASES.update({
    'low_mask': ((24, 32, 128, 67, 1), dict(vol_scale=2e-6)),
    'long_runs': ((24, 32, 128, 67, 1), dict(span=0.02)),
    'one_cell_waves': ((24, 32, 64, 5, 1), dict(zero_dirs=True)),
    'G34_grid_stride': ((2, 34, 64, 4100, 1), {}),          # P = 262 400 >= 65536 on global atomics, 1025 -> 1024 blocks
})
LDS_CASES = {
    'P65536': ((24, 32, 64, 1024, 1), {}),
    'B1': ((1, 32, 64, 1024, 1), {}),
    'G33_ragged': ((3, 33, 50, 1311, 1), {}),
    'B25_S2': ((25, 31, 2, 32769, 1), {}),
    # 100 bones x 3 axes x 2e-4 cell: delta = 1e-4 would zero 5.4 .. 5.8 % of the samples whatever the seed.  fp32 rounding
    # of a lattice coordinate grows with G (about 1e-5 at G = 32, 5e-6 here): 5e-5 keeps the same tenfold margin over it
    'B100_G16': ((100, 16, 128, 513, 1), dict(delta=5e-5)),
    'G2': ((24, 2, 64, 1024, 1), {}),
    'long_runs': ((24, 32, 128, 520, 1), dict(span=0.02)),
    'low_mask': ((24, 32, 64, 1024, 1), dict(vol_scale=2e-6)),
}
BELOW_SWITCH = ('P65535', ((24, 32, 15, 4369, 1), {}))        # same kind of problem, one sample below the LDS path
# Seeds other than 1.  dL/dw_b is the difference of two terms of size |g_x| |pos| / den, so a sample's rounding error grows
# with 1 / den.  In a case of a few hundred samples ONE sample with a weight sum in [1e-4, 0.1) carries as much error as
# all the others together (their weight sums are 1.5 with three bones and more with more: ten times less each, sqrt(250)
# = 16 times more in sum), and the floor is then one draw of one sample's rounding, not a yardstick: on the 256-sample
# case with seed 1 (one sample at 2.7e-3) two fp32 evaluations of the same formulas, the oracle's and the twin's, are
# 1.0e-5 and 8.1e-5 away from fp64 on that sample, the kernel 5.1e-5 in all (3.85 x the floor); on the 255-sample case
# with seed 2 (one sample at 2.2e-2) the kernel is at 3.59 x the floor.  The cases under 1000 samples therefore take the
# first seed without such a sample (test_small_cases_have_no_lone_ill_conditioned_sample: from the fp64 forward
# alone).  The regime itself is covered where it is not alone: the cases of thousands of samples, and the low-volume
# cases, whose every sample has den = 1e-4.
SEEDS = {'global-' + _name((4, 16, 7, 9, 1)): 3, 'global-' + _name((5, 31, 64, 5, 1)): 2, 'global-' + _name((24, 31, 7, 37, 1)): 2,
         'global-' + _name((25, 64, 129, 4, 1)): 2, 'global-edge_P255': 4, 'global-edge_P256': 3}
LONE_SAMPLE_CASES, ILL_CONDITIONED_BELOW = 1000, 0.1
ALL_CASES = {'global-' + k: v for k, v in GLOBAL_CASES.items()}
ALL_CASES.update({'lds-' + k: v for k, v in LDS_CASES.items()})
ALL_CASES['global-' + BELOW_SWITCH[0]] = BELOW_SWITCH[1]
SMALL_CASES = [k for k, (c, kw) in ALL_CASES.items() if c[2] * c[3] * c[0] <= 300000]


def takes_lds_path(pr):
    return pr['P'] >= LDS_MIN_SAMPLES and pr['G'] <= LDS_MAX_G


@functools.lru_cache(maxsize=None)
def problem(name):
    case, kw = ALL_CASES[name]
    return k1_bwd_problem(case, seed=SEEDS.get(name, 1), **kw)


@functools.lru_cache(maxsize=None)
def references(name):
    """(problem, fp64 reference, fp32 evaluation) of one case of ALL_CASES, computed once per process."""
    pr = problem(name)
    return pr, ref_k1_bwd(pr, torch.float64), ref_k1_bwd(pr, torch.float32)


def errors(got, ref64, ref32):
    """Per output: (max |got - ref64|, tolerance, floor)."""
    out = {}
    for k in ('vol', 'Rs', 'Ts'):
        tol, floor = refs.tolerance(ref32[k], ref64[k])
        g = torch.as_tensor(got[k]).double().reshape(ref64[k].shape)
        out[k] = (float((g - ref64[k]).abs().max()), tol, floor)
    return out


# ------------------------------------------------------------------------------------------------ checks (no GPU)
@pytest.mark.parametrize('name', SMALL_CASES)
def test_twin_agrees_with_fp64_autograd(name):
    pr, r64, r32 = references(name)
    for k, (err, tol, floor) in errors(k1_bwd_twin(pr), r64, r32).items():
        assert err <= tol, (name, k, err, tol)


def test_fp64_autograd_agrees_with_finite_differences():
    """B = 3, G = 5, R = 4, S = 3 (fewer than 9 rays: refs.k1_problem plants no far-outside ray), central differences of
    step 1e-6 in fp64 on a handful of entries of vol, Rs and Ts.  The samples with a gradient are 1e-4 cell from every
    face and 1e-6 from the clamp: a step of 1e-6 carries none of them across."""
    pr = k1_bwd_problem((3, 5, 3, 4, 1))
    assert not pr['zeroed'].all()
    g = ref_k1_bwd(pr)
    pts, gx, gm = _points(pr), _t(pr['g_x']), _t(pr['g_mask'])

    def loss(vol, Rs, Ts):
        x, m, _ = oracle.sample_motion_fields(pts, Rs, Ts, vol, _t(pr['bmin']), _t(pr['bscale']))
        return float((x * gx).sum() + (m * gm).sum())

    leaves = dict(vol=_t(pr['vol'])[:4], Rs=_t(pr['Rs']), Ts=_t(pr['Ts']))
    rs, h = np.random.RandomState(0), 1e-6
    for k in ('vol', 'Rs', 'Ts'):
        n = g[k].numel()
        picks = rs.choice(n, min(n, 12), replace=False) if k != 'vol' else torch.topk(g[k].abs().reshape(-1), 12).indices.numpy()
        scale = float(g[k].abs().max())
        for i in picks:
            d = []
            for s in (1, -1):
                a = {kk: v.clone() for kk, v in leaves.items()}
                a[k].reshape(-1)[i] += s * h
                d.append(loss(a['vol'], a['Rs'], a['Ts']))
            fd = (d[0] - d[1]) / (2 * h)
            assert abs(fd - float(g[k].reshape(-1)[i])) <= 1e-7 * scale, (k, int(i), fd, float(g[k].reshape(-1)[i]))


@pytest.mark.parametrize('name', list(ALL_CASES))
def test_zeroed_share_is_capped(name):
    pr = problem(name)
    share = float(pr['zeroed'].mean())
    print('ZEROED %s %.4f' % (name, share))
    assert share <= MAX_ZEROED, (name, share)


@pytest.mark.parametrize('name', [k for k, (c, kw) in ALL_CASES.items() if c[2] * c[3] < LONE_SAMPLE_CASES])
def test_small_cases_have_no_lone_ill_conditioned_sample(name):
    pr = problem(name)
    m = pr['mask64']
    assert not ((m >= 1e-4) & (m < ILL_CONDITIONED_BELOW) & ~pr['zeroed']).any(), name


def test_exact_lattice_problems_need_no_filter():
    """refs.k1_exact_problem: every sample is a node or a midpoint in exact fp32 arithmetic, so the fp32 and the fp64
    evaluation choose the same cell, face or not; most of its samples ARE on faces."""
    pr, _ = refs.k1_exact_problem(0, 7)
    p = k1_bwd_problem((7, 33, 33, pr['R'], 1), base=pr, filtered=False)
    assert face_filter(p).mean() > 0.8 and not p['zeroed'].any()


def test_low_mask_cases_run_the_clamped_branch():
    """Every weight sum of the two low-volume cases lies below the 1e-4 clamp, and more than half of them (the samples
    inside the volume and outside its empty slab) are positive: non-zero weights on the clamped-denominator branch."""
    for name in ('global-low_mask', 'lds-low_mask'):
        m = problem(name)['mask64']
        assert m.max() < 1e-4 and (m > 0).mean() > 0.5


@pytest.mark.parametrize('fault', TWIN_FAULTS)
def test_planted_faults_are_caught(fault):
    """Each planted fault pushes the twin outside the tolerance of at least one output on a case of >= 2000 samples."""
    name = {'low_mask_term': 'global-low_mask',                                  # every weight sum below the clamp
            'drop_last_partial_wave': 'global-' + _name((7, 33, 129, 37, 3))      # 4773 samples = 74 waves + 37
            }.get(fault, 'global-' + _name((24, 32, 128, 67, 1)))
    pr, r64, r32 = references(name)
    assert pr['P'] >= 2000 and (pr['P'] % 64 != 0 or fault != 'drop_last_partial_wave')
    e = errors(k1_bwd_twin(pr, fault), r64, r32)
    print('FAULT %s ' % fault + ' '.join('%s %.1f' % (k, err / floor) for k, (err, tol, floor) in e.items()))
    assert any(err > tol for err, tol, floor in e.values()), (fault, e)


# measured on the CPU: 3.4e-3 (d_Rs), 1.3e-2 (d_Ts) of the largest entry unfiltered; 3.9e-6, 2.0e-6 filtered.  Asserted: x 4
GRAD_SUITE_FLOOR = dict(Rs=1.6e-5, Ts=8e-6)


def test_filter_removes_the_face_flip_noise():
    """The 1100 x 64, G = 32 case of test_sample_warp_bwd_kernel: the oracle's fp32 autograd against its fp64 autograd,
    relative to the largest entry, with and without the face filter."""
    rel = {}
    for filtered in (False, True):
        pr = grad_suite_problem(1100, 32, 64, 0.5, filtered)
        r64, r32 = ref_k1_bwd(pr, torch.float64), ref_k1_bwd(pr, torch.float32)
        rel[filtered] = {k: float((r32[k].double() - r64[k]).abs().max() / r64[k].abs().max()) for k in ('vol', 'Rs', 'Ts')}
        print('FLOOR filtered=%s zeroed %.4f ' % (filtered, pr['zeroed'].mean()) + ' '.join('%s %.2e' % kv for kv in rel[filtered].items()))
    assert pr['zeroed'].mean() <= MAX_ZEROED
    for k in ('Rs', 'Ts'):
        assert rel[True][k] <= GRAD_SUITE_FLOOR[k], (k, rel)
