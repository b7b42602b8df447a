"""hnrf_sample_warp_bwd (K1') against fp64 torch.autograd through the oracle, on both of its forms: 256 threads with
global float atomics below 65536 samples (and for lattices whose gradient grid does not fit the reserved LDS), 1024
threads with the bone's G^3 gradient grid in LDS from there on.

Problems, references, the face filter and the case table: tests/test_warp_bwd_refs.py (checked there without a GPU).
Every comparison is max |kernel - fp64| <= 4 x the error of the reference's own fp32 evaluation on the same inputs (at
least 2e-7 of the output's largest entry), per output; nothing here is scaled by what the kernel returns.  Every test
prints its ratio of kernel error to that floor (``pytest -s``; profiles/k1_bwd_accuracy.txt has the values of one run).
tests/test_gpu_grad.py::test_sample_warp_bwd_kernel remains the unfiltered statement (3e-2: the reference's face-flip
noise)."""
import numpy as np
import pytest
import torch

from tests import test_render_kernel_refs as refs
from tests import test_warp_bwd_refs as wrefs

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _run(pr):
    """The kernel on a problem of wrefs.k1_bwd_problem: dict(vol (bone channels), Rs, Ts, rest (the other channels))."""
    from humannerf_amd import ops
    d_vol, d_Rs, d_Ts = ops.sample_warp_bwd(*(T(pr[k]) for k in ('rays_o', 'rays_d', 'z', 'Rs', 'Ts', 'vol', 'bmin', 'bscale',
                                                                  'x_skel', 'fg_mask', 'g_x', 'g_mask')))
    torch.cuda.synchronize()
    B = pr['B']
    assert d_vol.shape[0] == B + pr['extra']
    return dict(vol=d_vol[:B].cpu(), Rs=d_Rs.cpu(), Ts=d_Ts.cpu(), rest=d_vol[B:].cpu())


def _check(tag, got, r64, r32):
    bad = []
    for k, (err, tol, floor) in wrefs.errors(got, r64, r32).items():
        print('RATIO %s %s err %.3e floor %.3e ratio %.2f' % (tag, k, err, floor, err / floor if floor else 0.0))
        assert bool(torch.isfinite(got[k]).all()), (tag, k)
        if err > tol:
            bad.append((k, err, tol, floor))
    assert bool((got['rest'] == 0).all()), tag                  # the channels beyond the bones are never written
    assert not bad, (tag, bad)


def _against_fp64(name):
    pr, r64, r32 = wrefs.references(name)
    _check(name, _run(pr), r64, r32)
    return pr


GLOBAL = ['global-' + k for k in wrefs.GLOBAL_CASES] + ['global-' + wrefs.BELOW_SWITCH[0]]
LDS = ['lds-' + k for k in wrefs.LDS_CASES]


@pytest.mark.parametrize('name', GLOBAL)
def test_global_atomics_path_against_fp64(name):
    """<false, 256>: every geometry of refs.K1_CASES (bone counts 1 .. 25, lattices 2 .. 64 even and odd, 2 .. 257 samples
    per ray, 2 and 3 channels beyond the bones; a zero-length ray, a ray at 1e6, a zero direction, an empty slab); sample
    counts 63 / 64 / 65 and 255 / 256 / 257 (wave and block edges) and 2; weight sums below the 1e-4 clamp with non-zero
    weights; rays that stay in one cell for tens of samples, and waves whose 64 lanes all sit in one cell (the fold of
    same-cell lanes before the atomic); 65535 samples, one below the switch; and G = 34 at 262 400 samples, whose grid
    does not fit the LDS reserved for the other form: 1025 blocks' worth of samples on a grid capped at 1024."""
    pr = _against_fp64(name)
    assert not wrefs.takes_lds_path(pr)
    if name.endswith('low_mask'):
        _assert_low_mask(pr)
    if name.endswith('one_cell_waves'):
        assert not pr['rays_d'].any() and pr['S'] == 64


@pytest.mark.parametrize('name', LDS)
def test_lds_path_against_fp64(name):
    """<true, 1024>: exactly 65536 samples; one bone (the blocks per bone are capped by the sample count: whole waves lie
    beyond P); G = 33, the largest and an odd LDS lattice, 65550 samples of 50 per ray (ragged last wave, rays change
    inside the groups of 8 lanes); 25 bones of 2 samples per ray; 100 bones (5 blocks per bone, 13 ragged grid-stride
    trips); G = 2 (every sample on the same 8 voxels); long same-cell runs; weight sums below the clamp."""
    pr = _against_fp64(name)
    assert wrefs.takes_lds_path(pr)
    if name.endswith('low_mask'):
        _assert_low_mask(pr)


def _assert_low_mask(pr):
    """Every weight sum of the fp64 forward lies below the clamp, and those inside the volume (more than half) above 0."""
    m = pr['mask64']
    assert float(m.max()) < 1e-4 and float((m > 0).mean()) > 0.5


@pytest.mark.parametrize('B', [24, 7])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_exact_lattice_against_fp64(axis, B):
    """refs.k1_exact_problem, unfiltered: every sample is a lattice node or a midpoint in exact fp32 arithmetic, so the
    kernel and the fp64 autograd choose the same cell and the one-sided derivatives must agree; corners outside the grid
    on both sides."""
    base, lat = refs.k1_exact_problem(axis, B)
    pr = wrefs.k1_bwd_problem((B, 33, 33, base['R'], 1), base=base, filtered=False)
    assert (lat < 0).any() and (lat > 32).any() and not pr['zeroed'].any()
    _check('exact axis%d B%d' % (axis, B), _run(pr), wrefs.ref_k1_bwd(pr), wrefs.ref_k1_bwd(pr, torch.float32))


@pytest.mark.parametrize('name', ['global-' + wrefs._name((7, 33, 129, 37, 3)), 'lds-G33_ragged'])
def test_zero_gradient_gives_exact_zeros(name):
    pr = dict(wrefs.problem(name))
    pr['g_x'], pr['g_mask'] = np.zeros_like(pr['g_x']), np.zeros_like(pr['g_mask'])
    got = _run(pr)
    for k in ('vol', 'Rs', 'Ts', 'rest'):
        assert bool((got[k] == 0).all()), (name, k)


def test_paths_add_up_across_the_switch():
    """(24, 32, 64, 1024): the 1024 rays run on the LDS form, rays 0 .. 511 and 512 .. 1023 (32768 samples each) on global
    atomics; the gradient is a sum over samples, so the one result equals the sum of the other two within the sum of
    the three tolerances."""
    name = 'lds-P65536'
    whole, r64, r32 = wrefs.references(name)
    case, kw = wrefs.ALL_CASES[name]
    got, tol = _run(whole), {k: v[1] for k, v in wrefs.errors(r64, r64, r32).items()}
    assert wrefs.takes_lds_path(whole)
    parts = {k: torch.zeros_like(v) for k, v in got.items()}
    for rays in (slice(0, 512), slice(512, 1024)):
        pr = wrefs.k1_bwd_problem(case, rays=rays, **kw)
        assert not wrefs.takes_lds_path(pr) and pr['P'] == 32768
        h64, h32 = wrefs.ref_k1_bwd(pr), wrefs.ref_k1_bwd(pr, torch.float32)
        g = _run(pr)
        _check('half %d' % rays.start, g, h64, h32)
        for k, (_, t, _) in wrefs.errors(h64, h64, h32).items():
            tol[k] += t
            parts[k] += g[k]
    for k in ('vol', 'Rs', 'Ts'):
        err = float((got[k].double() - parts[k].double()).abs().max())
        print('RATIO additivity %s err %.3e tol %.3e' % (k, err, tol[k]))
        assert err <= tol[k], (k, err, tol[k])


def test_backward_of_the_forward_kernels_outputs():
    """As autograd.py chains them: ops.sample_warp, then ops.sample_warp_bwd on ITS z, x_skel and fg_mask (24, 32, 64,
    67).  Reference: fp64 autograd from that fp32 z; the face filter from the fp64 positions at that z."""
    from humannerf_amd import ops
    case = (24, 32, 64, 67, 1)
    geo = refs.k1_problem(*case)
    z, xs, mask, _ = ops.sample_warp(T(geo['rays_o']), T(geo['rays_d']), T(geo['near']), T(geo['far']), T(geo['t_rand']),
                                     T(geo['Rs']), T(geo['Ts']), T(geo['vol']), T(geo['bmin']), T(geo['bscale']), case[2])
    torch.cuda.synchronize()
    pr = wrefs.k1_bwd_problem(case, z=z.cpu().numpy(), x_skel=xs.cpu().numpy(), fg_mask=mask.cpu().numpy())
    assert pr['zeroed'].mean() <= wrefs.MAX_ZEROED
    _check('chained', _run(pr), wrefs.ref_k1_bwd(pr), wrefs.ref_k1_bwd(pr, torch.float32))
