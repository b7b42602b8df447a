"""Baked canonical grid without a GPU: the host twin of the sampler against an analytic field, its clamping, the
argument checks of the library, and the grid files."""
import numpy as np
import pytest
import torch

from humannerf_amd import baked, scene
from humannerf_amd.mesh import lattice_axes


def box():
    fr = scene.synthetic_frame(H=8, W=8)
    return fr['cnl_bbox_min_xyz'], fr['cnl_bbox_max_xyz']


# f_c(p) = A_c sin(a_c x + phi_c) cos(b_c y) sin(c_c z + 1/2): amplitudes up to 40, angular frequencies 1..5 per metre
AMP = np.array([1.0, 6.0, 17.0, 40.0])
FA = np.array([1.0, 2.5, 5.0, 3.0])
FB = np.array([5.0, 1.0, 3.0, 4.0])
FC = np.array([2.0, 5.0, 1.5, 4.5])
PHI = np.array([0.0, 0.7, 1.9, 3.1])


def field(p):
    p = np.asarray(p, dtype=np.float64)
    x, y, z = p[..., 0:1], p[..., 1:2], p[..., 2:3]
    return AMP * np.sin(FA * x + PHI) * np.cos(FB * y) * np.sin(FC * z + 0.5)


def analytic_grid(lo, hi, N):
    return field(baked.lattice_points(lo, hi, N)).astype(np.float16).reshape(N, N, N, 4)


@pytest.mark.parametrize('N', [32, 64, 128])
def test_interpolation_bound_on_an_analytic_field(N):
    """|sample - f| <= A (hx^2 a^2 + hy^2 b^2 + hz^2 c^2) / 8 + 2^-11 A + N 2^-22 A per channel.  First term: the
    remainder of tensor-product linear interpolation, sum over the axes of h^2 / 8 max|d^2 f / dx_i^2| (each
    one-dimensional interpolation operator has norm 1), with |d^2 f / dx^2| <= A a^2 etc.  Second: the stored values
    are rounded to f16, relative 2^-11 of |f| <= A, and interpolation is a convex combination.  Third: the float32
    coordinate u = (x - lo) * inv_step carries a relative rounding of a few 2^-24, i.e. up to ~N 2^-23 of a cell."""
    lo, hi = box()
    grid = analytic_grid(lo, hi, N)
    rs = np.random.RandomState(N)
    p = (lo + rs.uniform(0, 1, (200000, 3)) * (hi - lo)).astype(np.float32)
    p = np.clip(p, lo, hi)
    got = baked.sample_host(grid, p, lo, hi).astype(np.float64)
    h = (hi.astype(np.float64) - lo.astype(np.float64)) / (N - 1)
    bound = AMP * (h[0] ** 2 * FA ** 2 + h[1] ** 2 * FB ** 2 + h[2] ** 2 * FC ** 2) / 8 + 2.0 ** -11 * AMP + N * 2.0 ** -22 * AMP
    err = np.abs(got - field(p)).max(axis=0)
    print('N', N, 'max err / bound per channel', err / bound)
    assert np.all(err <= bound), (err, bound)
    # the bound is tight enough to catch a slip: a lattice off by one along x, or the x and z axes swapped
    for wrong in (np.roll(grid, 1, axis=2), np.ascontiguousarray(grid.transpose(2, 1, 0, 3))):
        bad = np.abs(baked.sample_host(wrong, p, lo, hi).astype(np.float64) - field(p)).max(axis=0)
        assert np.all(bad > bound), (bad, bound)


def test_sampler_is_exact_on_the_lattice_and_orders_the_axes():
    lo, hi = box()
    N = 16
    pts = baked.lattice_points(lo, hi, N)
    grid = np.zeros((N, N, N, 4), np.float16)
    ix, iy, iz = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing='ij')
    grid[iz, iy, ix, 0], grid[iz, iy, ix, 1], grid[iz, iy, ix, 2] = ix, iy, iz       # channel = index along x, y, z
    grid[..., 3] = 7.0
    got = baked.sample_host(grid, pts, lo, hi)
    want = np.stack([np.tile(np.arange(N), N * N), np.tile(np.repeat(np.arange(N), N), N), np.repeat(np.arange(N), N * N),
                     np.full(N ** 3, 7.0)], -1)
    assert np.abs(got - want).max() <= 1e-4
    ax = lattice_axes(lo, hi, N)
    assert np.array_equal(pts.reshape(N, N, N, 3)[3, 5, 7], np.array([ax[0][7], ax[1][5], ax[2][3]], np.float32))


def test_clamping_and_nan():
    lo, hi = box()
    N = 24
    grid = analytic_grid(lo, hi, N)
    rs = np.random.RandomState(1)
    p = (lo + rs.uniform(-0.6, 1.6, (50000, 3)) * (hi - lo)).astype(np.float32)
    outside = np.any((p < lo) | (p > hi), axis=1)
    assert outside.mean() > 0.5 and (~outside).sum() > 1000
    got = baked.sample_host(grid, p, lo, hi)
    assert np.array_equal(got.view(np.uint32), baked.sample_host(grid, np.clip(p, lo, hi), lo, hi).view(np.uint32))
    far = np.array([[1e30, -1e30, 0.0], [np.inf, -np.inf, np.inf]], np.float32)
    assert np.array_equal(baked.sample_host(grid, far, lo, hi), baked.sample_host(grid, np.clip(far, lo, hi), lo, hi))
    bad = p[:64].copy()
    bad[::2, 0], bad[1::3, 1], bad[::5, 2] = np.nan, np.nan, np.nan
    out = baked.sample_host(grid, bad, lo, hi)
    assert np.all(np.isfinite(out))
    allnan = np.full((1, 3), np.nan, np.float32)                      # a NaN coordinate samples index 0
    assert np.array_equal(baked.sample_host(grid, allnan, lo, hi)[0], grid[0, 0, 0].astype(np.float32))


def test_abi_rejects_bad_grids_without_a_gpu():
    from humannerf_amd import _lib
    lib = _lib.load()
    err = lambda: lib.hnrf_last_error().decode()
    assert lib.hnrf_baked_grid_bytes(7) == 0 and lib.hnrf_baked_grid_bytes(513) == 0
    assert lib.hnrf_baked_grid_bytes(256) == 256 ** 3 * 8
    assert lib.hnrf_bake_canonical_workspace_bytes(7) == 0
    assert lib.hnrf_bake_canonical_workspace_bytes(64) == lib.hnrf_density_grid_workspace_bytes(64) > 0
    assert lib.hnrf_baked_sample(None, None, 32, None, None, 10, None, None) == -1 and 'null' in err()
    assert lib.hnrf_baked_sample(16, 16, 32, None, 16, 10, 16, None) == -1 and 'null' in err()
    for N in (7, 513, 0, -1):
        assert lib.hnrf_baked_sample(16, 16, N, 16, 16, 10, 16, None) == -1 and 'out of range' in err()
        assert lib.hnrf_baked_sample_sparse(16, 16, N, 16, 16, 10, 16, 16, 16, None) == -1 and 'out of range' in err()
        assert lib.hnrf_bake_canonical(256, 1, 16, 16, N, 256, 1 << 40, 16, None, None) == -1 and 'out of range' in err()
    assert lib.hnrf_baked_sample_sparse(16, 16, 32, 16, 16, 10, None, 16, 16, None) == -1 and 'null' in err()
    assert lib.hnrf_baked_sample(16, 12, 32, 16, 16, 10, 16, None) == -1 and 'aligned' in err()
    assert lib.hnrf_bake_canonical(None, 1, 16, 16, 32, 256, 1 << 40, 16, None, None) == -1 and 'null' in err()
    assert lib.hnrf_bake_canonical(256, 7, 16, 16, 32, 256, 1 << 40, 16, None, None) == -2 and 'not built' in err()
    assert lib.hnrf_bake_canonical(256, 1, 16, 16, 32, 256, 16, 16, None, None) == -4 and 'workspace' in err()
    ws = 1 << 40
    frame = lambda grid, N: lib.hnrf_render_frame_baked_fwd(
        16, 16, 16, 16, None, 16, 16, 16, 16, 16, None, None, grid, N, 16, 16, 16, 1, 0.0, 100, 128, 24, 32, 64, 256, ws,
        16, 16, 16, None, None, None, None, None, None, None, None, None, None, None, None)
    assert frame(None, 32) == -1 and 'null grid' in err()
    assert frame(16, 600) == -1 and 'out of range' in err()
    rays = lambda grid, N: lib.hnrf_render_rays_baked_fwd(
        16, 16, 16, 16, None, 16, 16, 16, 16, 16, None, None, grid, N, 16, 16, 16, 1, 0.0, 100, 128, 24, 32, 256, ws,
        16, 16, 16, None, None, None)
    assert rays(None, 32) == -1 and 'null grid' in err()
    assert rays(16, 4) == -1 and 'out of range' in err()


def test_grid_files_round_trip_and_the_weight_hash_is_checked(tmp_path):
    from humannerf_amd.network import Network
    lo, hi = box()
    N = 12
    rs = np.random.RandomState(0)
    grid = rs.randn(N, N, N, 4).astype(np.float16)
    grid.reshape(-1)[:4] = [np.float16(65504), np.float16(-65504), np.float16(6e-8), np.float16(-0.0)]
    net = Network()
    h = net.canonical_weights_hash()
    path = str(tmp_path / 'avatar_grid.npz')
    baked.save_grid(path, grid, lo, hi, 'f16x3', weights_hash=h)
    back = baked.load_grid(path)
    assert back['grid'].dtype == np.float16 and np.array_equal(back['grid'].view(np.uint16), grid.view(np.uint16))
    assert np.array_equal(back['bbox_min'], lo) and np.array_equal(back['bbox_max'], hi)
    assert back['N'] == N and back['mode'] == 'f16x3' and back['weights_hash'] == h
    net.set_baked_grid(back['grid'], back['bbox_min'], back['bbox_max'], weights_hash=back['weights_hash'])
    assert net._kept['baked'].injected and torch.equal(net._kept['baked'].grid, torch.from_numpy(grid))
    with torch.no_grad():
        net.cnl_mlp.module.output_linear[0].bias[3] += 1.0
    assert net.canonical_weights_hash() != h
    with pytest.raises(ValueError, match='other canonical weights'):
        net.set_baked_grid(back['grid'], back['bbox_min'], back['bbox_max'], weights_hash=back['weights_hash'])
    net.set_baked_grid(back['grid'], back['bbox_min'], back['bbox_max'])          # no hash: the caller vouches
    with pytest.raises(ValueError):
        net.set_baked_grid(np.zeros((4, 4, 4, 4), np.float16), lo, hi)
    with pytest.raises(ValueError):
        baked.sample_host(grid.astype(np.float32), np.zeros((1, 3), np.float32), lo, hi)
    baked.save_grid(path, grid, lo, hi, 'f32')
    assert baked.load_grid(path)['weights_hash'] is None
