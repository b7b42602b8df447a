"""Baked non-rigid offset field without a GPU: the host twin of the fused sampler against a float64 restatement, the
convergence of the tabulated offsets to the fp64 oracle's MLP, the argument checks of the new entries, and the two new
cfg.amd keys."""
import numpy as np
import pytest
import torch

from humannerf_amd import baked, scene
from humannerf_amd.config import cfg, check_amd_options, get_cfg_defaults
from humannerf_amd.seeded import default_shapes, seeded_state

U0 = 2.0 ** -24                                                       # unit round-off of float32


def box():
    fr = scene.synthetic_frame(H=8, W=8)
    return fr['cnl_bbox_min_xyz'], fr['cnl_bbox_max_xyz']


def sample64(grid, p, lo, hi):
    """baked.sample_host's definition with every operation in float64 (grid values are exact in either)."""
    g = grid.astype(np.float64)
    N = g.shape[0]
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    idx, t = [], []
    for a in range(3):
        u = np.clip((p[:, a] - lo[a]) * ((N - 1) / (hi[a] - lo[a])), 0.0, N - 1.0)
        i0 = np.minimum(np.floor(u).astype(np.int64), N - 2)
        idx.append(i0)
        t.append((u - i0)[:, None])
    (ix, iy, iz), (tx, ty, tz) = idx, t
    d = []
    for dz in (0, 1):
        e = []
        for dy in (0, 1):
            a, b = g[iz + dz, iy + dy, ix], g[iz + dz, iy + dy, ix + 1]
            e.append(a + tx * (b - a))
        d.append(e[0] + ty * (e[1] - e[0]))
    return d[0] + tz * (d[1] - d[0])


def sample_bound(V, N, extent, dx):
    """Bound of |sample_host - sample64| for a grid with |values| <= V, when the float32 input is within dx of the
    float64 one (per axis).  Two parts.  Blend: a + t (b - a) is three float32 roundings, of b - a (|.| <= 2 V), of the
    product (<= 2 V) and of the sum (<= V): 5 V u0 per lerp; a lerp passes the errors of its inputs on as their convex
    combination, so the three levels (4 + 2 + 1 = 7 lerps) add up to 15 V u0.  Coordinate: u = (x - lo) * (n / (hi -
    lo)) carries three roundings, |du| <= 3 u0 n, and the input's dx n / extent; t = u - i0 is exact; the interpolant
    is continuous and piecewise linear in u with slope <= max |b - a| <= 2 V along every axis (clamping only lowers
    it).  A hundredth on top for the second-order terms."""
    n = N - 1
    return 1.01 * (15 * V * U0 + 2 * V * n * float(np.sum(3 * U0 + dx / extent)))


def test_host_twin_against_float64():
    lo, hi = box()
    extent = (hi - lo).astype(np.float64)
    rs = np.random.RandomState(5)
    M, N = 12, 20
    off_grid = np.zeros((M, M, M, 4), np.float16)
    off_grid[..., :3] = (0.05 * rs.randn(M, M, M, 3)).astype(np.float16)        # offsets of centimetres
    cnl_grid = (3.0 * rs.randn(N, N, N, 4)).astype(np.float16)
    x = (lo + rs.uniform(-0.2, 1.2, (20000, 3)) * (hi - lo)).astype(np.float32)  # a fifth of them outside the box
    raw, xyz, off = baked.warp_sample_host(off_grid, cnl_grid, x, (lo, hi))
    assert raw.dtype == xyz.dtype == off.dtype == np.float32
    assert raw.shape == (20000, 4) and xyz.shape == off.shape == (20000, 3)
    x64 = x.astype(np.float64)
    off64 = sample64(off_grid, x64, lo, hi)[:, :3]
    xyz64 = x64 + off64
    raw64 = sample64(cnl_grid, xyz64, lo, hi)
    V_off, V_cnl = float(np.abs(off_grid.astype(np.float64)).max()), float(np.abs(cnl_grid.astype(np.float64)).max())
    tol_off = sample_bound(V_off, M, extent, 0.0)
    tol_xyz = tol_off + U0 * float(np.abs(xyz64).max())                          # the one add per coordinate
    tol_raw = sample_bound(V_cnl, N, extent, tol_xyz)
    err = [float(np.abs(a - b).max()) for a, b in ((off, off64), (xyz, xyz64), (raw, raw64))]
    print('max err off %.3e (tol %.3e), xyz %.3e (%.3e), raw %.3e (%.3e)'
          % (err[0], tol_off, err[1], tol_xyz, err[2], tol_raw))
    assert err[0] <= tol_off and err[1] <= tol_xyz and err[2] <= tol_raw
    assert err[2] > 0.0                                                          # (float32 it is)
    # the tolerance catches a slip: the offset grid's axes swapped, or the offsets left out
    bad, _, _ = baked.warp_sample_host(np.ascontiguousarray(off_grid.transpose(2, 1, 0, 3)), cnl_grid, x, (lo, hi))
    assert float(np.abs(bad - raw64).max()) > 100 * tol_raw
    assert float(np.abs(baked.sample_host(cnl_grid, x, lo, hi) - raw64).max()) > 100 * tol_raw
    # one box for both grids, or one per grid
    lo2, hi2 = lo - np.float32(0.125), hi + np.float32(0.25)
    two, _, _ = baked.warp_sample_host(off_grid, cnl_grid, x, ((lo, hi), (lo2, hi2)))
    _, xyz1, _ = baked.warp_sample_host(off_grid, cnl_grid, x, ((lo, hi), (lo, hi)))
    assert np.array_equal(xyz1.view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(two.view(np.uint32), baked.sample_host(cnl_grid, xyz, lo2, hi2).view(np.uint32))


def test_constant_and_zero_offset_grids():
    lo, hi = box()
    rs = np.random.RandomState(6)
    M, N = 9, 16
    cnl_grid = rs.randn(N, N, N, 4).astype(np.float16)
    x = (lo + rs.uniform(-0.3, 1.3, (5000, 3)) * (hi - lo)).astype(np.float32)
    x[::11, 1] = np.nan
    c = np.array([0.25, -0.125, 0.5, 0.0], np.float16)
    const = np.broadcast_to(c, (M, M, M, 4)).copy()
    raw, xyz, off = baked.warp_sample_host(const, cnl_grid, x, (lo, hi))
    assert np.array_equal(off, np.broadcast_to(c[:3].astype(np.float32), off.shape))       # a + t (a - a) = a
    with np.errstate(invalid='ignore'):
        want = x + c[:3].astype(np.float32)
    assert np.array_equal(xyz.view(np.uint32), want.view(np.uint32))
    assert np.all(np.isfinite(raw))                                   # a NaN coordinate samples index 0
    zero = np.zeros((M, M, M, 4), np.float16)
    raw0, xyz0, off0 = baked.warp_sample_host(zero, cnl_grid, x, (lo, hi))
    assert not off0.any() and np.array_equal(xyz0.view(np.uint32), x.view(np.uint32))
    assert np.array_equal(raw0.view(np.uint32), baked.sample_host(cnl_grid, x, lo, hi).view(np.uint32))


def test_the_offset_grid_converges_to_the_oracle():
    """The experiment behind the feature in small: the fp64 oracle's non-rigid MLP of the seeded network in the pose
    of synthetic_frame(pose_seed=3, pose_scale=0.3), tabulated in f16 on M^3 lattices over the canonical box and
    interpolated by the host twin at 5 000 uniform points.  Trilinear error falls with h^2 on a smooth field (the
    encoding stops at 2^5): 16x from M = 16 to 64 where the asymptotic rate holds, measured ratio 0.18 (the coarse
    lattice under-samples the top octave).  Asked: below a half."""
    from oracle import oracle
    state = {k: torch.from_numpy(v).double() for k, v in seeded_state(default_shapes(), 0).items()}
    fr = scene.synthetic_frame(64, 64, pose_seed=3, pose_scale=0.3)
    lo, hi = fr['cnl_bbox_min_xyz'], fr['cnl_bbox_max_xyz']
    nr = cfg.non_rigid_motion_mlp
    hw = oracle.hann_weights(1e7, nr.multires, nr.kick_in_iter, nr.full_band_iter, torch.float64)
    cond = torch.from_numpy(fr['dst_posevec']).double().reshape(1, -1)

    def offsets(p):
        x = torch.from_numpy(np.ascontiguousarray(p)).double()
        with torch.no_grad():
            return oracle.non_rigid_mlp(state, oracle.hann_pe(x, hw), cond, x)[1].numpy()

    rs = np.random.RandomState(0)
    pts = (lo + rs.uniform(0, 1, (5000, 3)) * (hi - lo)).astype(np.float32)
    exact = offsets(pts)
    err = {}
    for M in (16, 64):
        grid = np.zeros((M, M, M, 4), np.float16)
        grid[..., :3] = offsets(baked.lattice_points(lo, hi, M)).astype(np.float16).reshape(M, M, M, 3)
        got = baked.sample_host(grid, pts, lo, hi)
        assert not got[:, 3].any()
        err[M] = float(np.abs(got[:, :3] - exact).max())
    print('max |d offset| (m): M=16 %.3e, M=64 %.3e, ratio %.3f; max |offset| %.3e'
          % (err[16], err[64], err[64] / err[16], np.abs(exact).max()))
    assert err[16] > 100 * 2.0 ** -11 * float(np.abs(exact).max())   # (well above the f16 rounding of the values)
    assert err[64] < 0.5 * err[16]


def test_abi_rejects_bad_arguments_without_a_gpu():
    from humannerf_amd import _lib
    lib = _lib.load()
    err = lambda: lib.hnrf_last_error().decode()
    assert lib.hnrf_abi_version() == 13
    assert lib.hnrf_bake_nonrigid_workspace_bytes(7) == 0 and lib.hnrf_bake_nonrigid_workspace_bytes(513) == 0
    assert lib.hnrf_bake_nonrigid_workspace_bytes(32) == 3 * 32 ** 3 * 12
    assert lib.hnrf_bake_nonrigid_workspace_bytes(512) == 3 * (1 << 21) * 12          # chunks of 2^21 lattice points
    big = 1 << 40
    bake = lambda packed=256, hann=16, mode=1, lo=16, hi=16, M=32, ws=256, nbytes=big, grid=16: \
        lib.hnrf_bake_nonrigid(packed, hann, mode, lo, hi, M, ws, nbytes, grid, None, None)
    for kw in ({'packed': None}, {'hann': None}, {'ws': None}, {'grid': None}, {'lo': None}, {'hi': None}):
        assert bake(**kw) == -1 and 'null' in err(), kw
    for M in (7, 513, 0, -1):
        assert bake(M=M) == -1 and 'out of range' in err()
    assert bake(grid=12) == -1 and 'aligned' in err()
    assert bake(ws=128) == -1 and 'aligned' in err()
    assert bake(mode=7) == -2 and 'not built' in err()
    assert bake(nbytes=16) == -4 and 'workspace' in err()

    def warp(x=16, og=16, M=32, olo=16, ohi=16, cg=16, N=32, clo=16, chi=16, P=10, raw=16, sparse=False, idx=16, cnt=16):
        if sparse:
            return lib.hnrf_baked_warp_sample_sparse(x, og, M, olo, ohi, cg, N, clo, chi, P, idx, cnt, raw, None, None, None)
        return lib.hnrf_baked_warp_sample(x, og, M, olo, ohi, cg, N, clo, chi, P, raw, None, None, None)
    for sparse in (False, True):
        for kw in ({'x': None}, {'og': None}, {'olo': None}, {'ohi': None}, {'cg': None}, {'clo': None}, {'chi': None},
                   {'raw': None}):
            assert warp(sparse=sparse, **kw) == -1 and 'null' in err(), kw
        for bad in (7, 513, 0, -1):
            assert warp(sparse=sparse, M=bad) == -1 and 'out of range' in err()
            assert warp(sparse=sparse, N=bad) == -1 and 'out of range' in err()
        assert warp(sparse=sparse, og=12) == -1 and 'aligned' in err()
        assert warp(sparse=sparse, cg=20) == -1 and 'aligned' in err()
        assert warp(sparse=sparse, raw=24) == -1 and 'aligned' in err()
        assert warp(sparse=sparse, P=-1) == -1 and 'bad P' in err()
    assert warp(sparse=True, idx=None) == -1 and 'null' in err()
    assert warp(sparse=True, cnt=None) == -1 and 'null' in err()

    frame = lambda og=16, M=32, cg=16, N=64, olo=16: lib.hnrf_render_frame_baked_nr_fwd(
        16, 16, 16, 16, None, 16, 16, 16, 16, 16, og, M, olo, 16, cg, N, 16, 16, 16, 1, 0.0, 100, 128, 24, 32, 64, 256, big,
        16, 16, 16, None, None, None, None, None, None, None, None, None, None, None, None)
    rays = lambda og=16, M=32, cg=16, N=64, olo=16: lib.hnrf_render_rays_baked_nr_fwd(
        16, 16, 16, 16, None, 16, 16, 16, 16, 16, og, M, olo, 16, cg, N, 16, 16, 16, 1, 0.0, 100, 128, 24, 32, 256, big,
        16, 16, 16, None, None, None)
    for fn in (frame, rays):
        assert fn(og=None) == -1 and 'null offset grid' in err()
        assert fn(cg=None) == -1 and 'null grid' in err()
        assert fn(olo=None) == -1 and 'null' in err()
        assert fn(M=600) == -1 and 'out of range' in err()
        assert fn(M=4) == -1 and 'out of range' in err()
        assert fn(N=7) == -1 and 'out of range' in err()
        assert fn(og=12) == -1 and 'aligned' in err()
        assert fn(cg=12) == -1 and 'aligned' in err()


def test_config_keys_and_their_validation():
    c = get_cfg_defaults()
    assert c.amd.nonrigid == 'mlp' and c.amd.nonrigid_bake_resolution == 128
    assert check_amd_options(c.amd) == ('mlp', 'mlp', 128)
    c.amd.canonical, c.amd.nonrigid, c.amd.nonrigid_bake_resolution = 'baked', 'baked', 64
    assert check_amd_options(c.amd) == ('baked', 'baked', 64)
    c.amd.canonical = 'mlp'
    with pytest.raises(ValueError) as e:
        check_amd_options(c.amd)
    assert 'cfg.amd.nonrigid' in str(e.value) and 'cfg.amd.canonical' in str(e.value)
    c.amd.canonical = 'baked'
    for bad in ('grid', None, 1):
        c.amd.nonrigid = bad
        with pytest.raises(ValueError, match='cfg.amd.nonrigid must be'):
            check_amd_options(c.amd)
    c.amd.nonrigid = 'baked'
    for bad in (7, 513, 0, -128, 64.0, '128', True):
        c.amd.nonrigid_bake_resolution = bad
        with pytest.raises(ValueError, match='nonrigid_bake_resolution'):
            check_amd_options(c.amd)
    c.amd.nonrigid_bake_resolution = 8
    assert check_amd_options(c.amd)[2] == 8
    c.amd.canonical = 'sparse'
    with pytest.raises(ValueError, match='cfg.amd.canonical must be'):
        check_amd_options(c.amd)
    # the process-wide cfg is at its defaults: the option is off
    assert check_amd_options()[1] == cfg.amd.get('nonrigid', 'mlp')


def test_network_refuses_baked_offsets_without_a_baked_canonical():
    """Option handling of Network.forward, without a GPU: the inconsistent pair raises before anything is launched."""
    from humannerf_amd.network import Network
    net = Network().eval()
    assert net.nonrigid_bake_count == 0 and 'baked_nr' not in net._kept
    fr = scene.synthetic_frame(H=8, W=8)
    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
            'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']
    old = (cfg.amd.get('canonical'), cfg.amd.get('nonrigid'))
    cfg.amd.canonical, cfg.amd.nonrigid = 'mlp', 'baked'
    try:
        with torch.no_grad(), pytest.raises(ValueError) as e:
            net(**{k: torch.from_numpy(np.ascontiguousarray(fr[k])) for k in keys})
        assert 'cfg.amd.nonrigid' in str(e.value) and 'cfg.amd.canonical' in str(e.value)
    finally:
        cfg.amd.canonical, cfg.amd.nonrigid = old
    assert net.nonrigid_bake_count == 0
