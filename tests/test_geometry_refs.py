"""Geometry maps without a GPU (include/hnrf_geometry.h, humannerf_amd/geometry.py): the numpy twins against independent
statements -- analytic surfaces seen by a pinhole camera, a sequential fp64 cumulative sum, the reference's own offset
colour map (tests/golden/geometry_offsets.npz, tests/make_golden_geometry.py) -- and the library's exports and refusals.
The GPU file (tests/test_gpu_geometry.py) compares the kernels with these twins bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import geometry_cases as gc
from humannerf_amd import geometry as geo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float32).eps)


def _maps(o, d, surf, p2r, H, W, want=('normal', 'nvalid'), **kw):
    kw.setdefault('bgcolor', (0.0, 0.0, 0.0))
    return geo.maps_host(o, d, surf, p2r, H, W, want=want, **kw)


def _facing(n, d):
    """The unit normal ``n`` turned towards the camera of the rays ``d``."""
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    return np.where(((d * n).sum(-1) > 0)[..., None], -n, n)


# ---------------------------------------------------------------------------------------------------- tilted planes
FLOOR_REL, TOL_FACTOR = 2e-7, 4.0       # tests/test_render_kernel_refs.py: 4 x max(fp32-vs-fp64 error, 2e-7 x scale)


def _reference_normals(n, H, W, dtype):
    """The statement the twin is held against, in ``dtype`` from the camera on: the ray / plane intersection, the point
    P = o + d t, central differences, cross product, normalisation.  Interior pixels, (H - 2, W - 2, 3), facing the
    camera; and the points' largest coordinate over the shortest difference (the scale of an angle error)."""
    o, d = (v.astype(dtype) for v in gc.camera(H, W))
    nn = np.asarray(n, dtype)
    t = (-(o * nn).sum(1, dtype=dtype)) / (d * nn).sum(1, dtype=dtype)
    P = (o + d * t[:, None]).reshape(H, W, 3)
    A, B = P[1:-1, 2:] - P[1:-1, :-2], P[2:, 1:-1] - P[:-2, 1:-1]
    c = np.stack([A[..., 1] * B[..., 2] - A[..., 2] * B[..., 1], A[..., 2] * B[..., 0] - A[..., 0] * B[..., 2],
                  A[..., 0] * B[..., 1] - A[..., 1] * B[..., 0]], -1)
    c = c / np.sqrt((c * c).sum(-1, dtype=dtype))[..., None]
    dd = d.reshape(H, W, 3)[1:-1, 1:-1]
    c = np.where(((c * dd).sum(-1) > 0)[..., None], -c, c)
    assert c.dtype == dtype
    scale = float(np.abs(P).max() / min(np.linalg.norm(A, axis=-1).min(), np.linalg.norm(B, axis=-1).min()))
    return c, scale


@pytest.mark.parametrize('n', gc.PLANES)
def test_tilted_plane_normals(n):
    """Every interior pixel of a plane has a normal, and its angle to the plane's normal is below 4 x the error of the
    same formula evaluated in fp32, the project's rule (tests/test_render_kernel_refs.py::tolerance, used by
    tests/test_mesh_kernel_refs.py): tolerance = 4 x max(error of the reference's own fp32 evaluation against fp64,
    2e-7 x scale).  The fp32 evaluation starts where the twin's inputs start -- the distance t is an fp32 number for
    both (on points rounded once from fp64 the formula's error is exactly 0 for the planes (0, 0, 1) and (1, 0, 1), a
    yardstick no fp32 distance can meet: half an ulp of t = 3 moves a point by 1.2e-7 over a baseline of 0.06).  The
    scale of an angle: a relative perturbation e of the points' coordinates turns a difference of length |D| by at most
    e max|P| / |D| radians.
    Measured: twin 0, 2.5e-4, 9.2e-5, 1.5e-4 degrees for the four planes, below the fp32 formula's own 0, 4.3e-4, 2.4e-4,
    2.4e-4 (profiles/geometry_maps.txt)."""
    H, W = 17, 33
    t64 = gc.plane_t(n, 0.0, H, W)
    assert (t64 > 0).all()
    o, d, surf, p2r = gc.full_frame(H, W, t64)
    res = _maps(o, d, surf, p2r, H, W, edge=1e9)
    assert res['nvalid'][1:-1, 1:-1].all()
    d64 = gc.camera(H, W)[1].reshape(H, W, 3)
    truth = _facing(n, d64)
    got = gc.angle_deg(res['normal'][1:-1, 1:-1], truth[1:-1, 1:-1]).max()
    n32, scale = _reference_normals(n, H, W, np.float32)
    n64, _ = _reference_normals(n, H, W, np.float64)
    assert gc.angle_deg(n64, truth[1:-1, 1:-1]).max() < 1e-9              # the fp64 statement is the plane's normal
    yard = gc.angle_deg(n32, n64).max()
    floor = max(yard, np.degrees(FLOOR_REL * scale))
    print('plane %r: twin %.3e deg, the formula in fp32 %.3e deg, floor %.3e deg' % (n, got, yard, floor))
    assert got < TOL_FACTOR * floor
    # the whole image has a normal too: the border takes the one-sided differences, over half the baseline
    assert res['nvalid'].all() and gc.angle_deg(res['normal'], truth).max() < 2 * TOL_FACTOR * floor


# ----------------------------------------------------------------------------------------------------------- sphere
def test_sphere_normals():
    """Sphere r = 0.5: every pixel whose true normal has -n.d^ > 0.5 has a normal, within 1 degree.  A numpy prototype of
    the rule gave 673 such pixels, max 0.66, mean 0.16 degrees."""
    H = W = 32
    t64, hit = gc.sphere_t(0.5, H, W)
    o, d, surf, p2r = gc.full_frame(H, W, t64, hit)
    res = _maps(o, d, surf, p2r, H, W, edge=0.05)
    o64, d64 = gc.camera(H, W)
    P = o64 + d64 * t64[:, None]
    n_true = P / np.linalg.norm(P, axis=1, keepdims=True)
    cosv = -(n_true * d64).sum(1) / np.linalg.norm(d64, axis=1)
    sel = (hit & (cosv > 0.5)).reshape(H, W)
    err = gc.angle_deg(res['normal'], n_true.reshape(H, W, 3))[sel]
    print('sphere: %d pixels, all with a normal %s, max %.3f deg, mean %.3f deg' % (sel.sum(), res['nvalid'][sel].all(),
                                                                                  err.max(), err.mean()))
    assert sel.sum() == 673
    assert res['nvalid'][sel].all()
    assert err.max() <= 1.0
    assert abs(err.max() - 0.66) < 0.01 and abs(err.mean() - 0.16) < 0.01
    assert not res['nvalid'][~hit.reshape(H, W)].any() and not res['normal'][~hit.reshape(H, W)].any()


# ------------------------------------------------------------------------------------------------------- depth step
def test_depth_step_takes_one_sided_differences():
    H, W, col = 9, 16, 8
    o, d, surf, p2r = gc.full_frame(H, W, gc.step_t(H, W, col))
    near = _maps(o, d, surf, p2r, H, W, edge=0.05)
    assert near['nvalid'].all()
    ang = gc.angle_deg(near['normal'], np.array([0.0, 0.0, 1.0]))
    assert ang.max() < 1e-3                                      # both planes, the columns beside the step included
    far = _maps(o, d, surf, p2r, H, W, edge=1.0)                 # the central difference straddles the step
    ang = gc.angle_deg(far['normal'], np.array([0.0, 0.0, 1.0]))
    assert ang[:, [col - 1, col]].min() > 30.0 and np.delete(ang, [col - 1, col], axis=1).max() < 1e-3


def test_one_pixel_island_has_no_normal_and_ambient_shade():
    H, W = 5, 7
    hit = np.zeros((H, W), bool)
    hit[2, 3] = True
    o, d, surf, p2r = gc.full_frame(H, W, np.full(H * W, 3.0), hit)
    res = _maps(o, d, surf, p2r, H, W, want=geo.OUTPUTS[:5], alpha=np.ones(H * W, np.float32), M=np.eye(3),
                lohi=(2.0, 4.0), bgcolor=(1.0, 0.0, 0.5))
    assert not res['nvalid'].any() and not res['normal'].any()
    assert res['shaded8'][2, 3].tolist() == [51, 51, 51]         # trunc(255 * 0.25 * 0.8)
    assert res['depth8'][2, 3].tolist() == [127, 127, 127]       # 1 - (3 - 2) / (4 - 2)
    bg = [255, 0, 127]
    assert res['normal8'][2, 3].tolist() == bg                   # no normal: the background
    for k in ('shaded8', 'depth8', 'normal8'):
        assert (res[k][~hit] == bg).all()


def test_pixel_rays_host():
    p, st = geo.pixel_rays_host([5, 0, 5, 2], 2, 3)
    assert st == 0 and p.tolist() == [1, -1, 3, -1, -1, 2]       # two rays on pixel 5: the highest wins
    assert geo.pixel_rays_host([0, 6], 2, 3) == (None, 1) and geo.pixel_rays_host([-1], 2, 3) == (None, 1)
    p, st = geo.pixel_rays_host([], 1, 1)
    assert st == 0 and p.tolist() == [-1]


# -------------------------------------------------------------------------------------------------- surface distance
@pytest.mark.parametrize('S', gc.S_LIST)
def test_ray_surface_against_sequential_fp64(S):
    """t_exp, the validity bits and the median sample against a sequential fp64 statement.  The median index must equal
    the fp64 one wherever fp64's c_k and c_{k-1} are further from the threshold than the scan's rounding bound: a sum
    of the scan passes through at most 6 additions inside its tile and one per tile for the carry, so
    |c_k - exact| <= depth * eps * c_k with depth = 6 + ceil(S / 64), and the same for the total that is halved; a
    margin of 1.5 * depth * eps * total covers both sides of the comparison.  The share of rays this excludes is
    printed and must stay below 1 % (measured: 0 to 0.07 %, one ray at S = 63 and at S = 300)."""
    R = 1500
    near, far, alpha, depth, w, off = gc.surface_inputs(R, S, seed=S)
    res = geo.ray_surface_host(near, far, alpha, depth, w, off, want_median=True, want_woff=True)
    ok = np.isfinite(alpha) & np.isfinite(depth) & (alpha >= np.float32(0.5))
    assert ok[7] and not ok[6] and not ok[8] and not ok[9]
    assert np.array_equal(res['valid'] & 1, ok.astype(np.uint8))
    want = (depth.astype(np.float64)[ok] / alpha.astype(np.float64)[ok]).astype(np.float32)      # one rounding: IEEE division
    assert np.array_equal(res['t_exp'][ok], want) and not res['t_exp'][~ok].any()
    # the special rows
    med = (res['valid'] >> 1) & 1
    assert not med[0] and not med[4] and not med[6]                         # zero weights, a NaN, alpha below alpha_min
    if S == 1:
        assert not med.any() and not res['t_med'].any()                     # z_at has no value at S = 1 (0 / 0)
        return
    assert res['k_med'][1] == 0 and res['k_med'][2] == S - 1 and res['k_med'][3] == (S + 1) // 2 - 1   # all ones: exact sums
    assert med[5] and res['t_med'][5] == near[5]                            # near == far
    c64 = np.cumsum(np.nan_to_num(w.astype(np.float64)), axis=1)           # sequential
    total = c64[:, -1]
    live = ok & (total > 0) & ~np.isnan(w).any(1)
    k64 = (c64 >= 0.5 * total[:, None]).argmax(1)
    bound = 1.5 * (6 + -(-S // 64)) * EPS * total
    rows = np.arange(R)
    below = np.where(k64 > 0, c64[rows, np.maximum(k64 - 1, 0)], -np.inf)
    sure = live & (c64[rows, k64] - 0.5 * total > bound) & (0.5 * total - below > bound)
    sure[3] = True                                                           # (all ones: every sum is an exact integer)
    excluded = (live & ~sure).mean()
    print('S %d: %d live rays, %.3f %% excluded by the bound' % (S, live.sum(), 100 * excluded))
    assert excluded < 0.01
    assert np.array_equal(res['k_med'][sure], k64[sure]) and med[sure].all()
    assert np.array_equal(res['k_med'] >= 0, med.astype(bool)) and (res['k_med'][~live] == -1).all()
    k = np.maximum(res['k_med'], 0)
    lin = np.linspace(0.0, 1.0, S)[k]
    z64 = near.astype(np.float64) * (1 - lin) + far.astype(np.float64) * lin
    sel = med.astype(bool)
    assert np.abs(res['t_med'][sel] - z64[sel]).max() <= 4 * EPS * far.max()
    assert not res['t_med'][~sel].any()


def test_lean_form_and_refusals_of_the_twin():
    near, far, alpha, depth, w, off = gc.surface_inputs(50, 16, seed=3)
    lean = geo.ray_surface_host(near, far, alpha, depth)
    full = geo.ray_surface_host(near, far, alpha, depth, w, off, want_median=True, want_woff=True)
    assert sorted(lean) == ['t_exp', 'valid'] and np.array_equal(lean['t_exp'], full['t_exp'])
    assert np.array_equal(lean['valid'], full['valid'] & 1)
    with pytest.raises(ValueError, match='weights'):
        geo.ray_surface_host(near, far, alpha, depth, want_median=True)
    with pytest.raises(ValueError, match='offsets'):
        geo.ray_surface_host(near, far, alpha, depth, w, want_woff=True)


# ----------------------------------------------------------------------------------------------- the reference's map
def test_woff_and_offset_colours_equal_the_reference():
    """woff: the header's order (one sample per lane at S = 16, then the butterfly) is not numpy's (row by row,
    ascending), so the two sums are compared within the bound of two orderings of the same S products,
    (S - 1) * eps * sum |w o|; the colour map is exact on the reference's own sum, and end to end differs by at most one
    level (where 255 v sits within that bound of an integer)."""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'geometry_offsets.npz'))
    w, off = z['weights'], z['offsets']
    S = w.shape[1]
    assert w.shape == (37, 16) and off.shape == (37, 16, 3)
    got = geo.weighted_offsets_host(w, off)
    bound = (S - 1) * EPS * np.abs(w[..., None].astype(np.float64) * off).sum(1)
    assert (np.abs(got.astype(np.float64) - z['woff']) <= bound).all()
    assert np.array_equal(geo.offset_color_host(z['woff']), z['color8'])
    assert np.abs(geo.offset_color_host(got).astype(int) - z['color8']).max() <= 1
    assert (z['color8'] == 0).any() and (z['color8'] == 255).any() and (z['color8'][1] == 127).all()
    # painted where the truth has colour, 0 elsewhere -- not the background
    H, W = 5, 8
    o, d, surf, p2r = gc.full_frame(H, W, np.full(H * W, 3.0))
    surf['woff'] = z['woff'][:H * W] if len(z['woff']) >= H * W else np.resize(z['woff'], (H * W, 3))
    truth = np.zeros((H, W, 3), np.uint8)
    truth[1:3, 2:5] = (0, 9, 0)
    res = _maps(o, d, surf, p2r, H, W, want=('offset8',), truth8=truth, bgcolor=(1.0, 1.0, 1.0))
    want = np.where((truth.sum(-1) > 0)[..., None], geo.offset_color_host(surf['woff']).reshape(H, W, 3), 0)
    assert np.array_equal(res['offset8'], want) and res['offset8'][0, 0].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ library and config
GEOMETRY_SYMBOLS = ['hnrf_geometry_maps', 'hnrf_pixel_rays', 'hnrf_ray_surface']


def test_geometry_entries_are_additive_to_abi_13():
    from humannerf_amd import _lib
    assert sorted(_lib.GEOMETRY_SIGNATURES) == GEOMETRY_SYMBOLS
    assert not set(_lib.GEOMETRY_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.CLOUD_SIGNATURES)
                                                | set(_lib.VIDEO_SIGNATURES) | set(_lib.SEGMENT_SIGNATURES))
    lib = _lib.load_geometry()                   # raises when the library lacks one of them
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in GEOMETRY_SYMBOLS:
        assert getattr(raw, name) is not None
    assert lib.hnrf_abi_version() == 13


def test_refusals_need_no_gpu():
    """Bad arguments are refused before any launch, and hnrf_last_error names the argument."""
    from humannerf_amd import _lib
    lib = _lib.load_geometry()
    err = lambda: lib.hnrf_last_error().decode()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    rs = lambda **k: lib.hnrf_ray_surface(*[k.get(a, p) for a in ('near', 'far', 'alpha', 'depth', 'weights', 'offsets')],
                                          k.get('R', 4), k.get('S', 4), k.get('alpha_min', 0.5),
                                          *[k.get(a, p) for a in ('t_exp', 't_med', 'woff', 'valid')], None)
    assert rs(S=0) != 0 and 'S 0' in err()
    assert rs(R=-1) != 0 and 'R -1' in err()
    assert rs(alpha_min=float('nan')) != 0 and 'alpha_min' in err()
    assert rs(weights=None) != 0 and 't_med needs weights' in err()
    assert rs(weights=None, offsets=None, t_med=None) != 0 and 'woff needs weights' in err()
    assert rs(offsets=None, t_med=None) != 0 and 'woff needs weights and offsets' in err()
    assert rs(near=None) != 0 and 'near' in err()
    assert rs(alpha=None) != 0 and 'null pointer' in err()
    pr = lambda idx=p, N=1, H=2, W=2, pix=p, st=p: lib.hnrf_pixel_rays(idx, N, H, W, pix, st, None)
    assert pr(H=0) != 0 and 'H 0' in err()
    assert pr(W=16385) != 0 and 'W 16385' in err()
    assert pr(N=1 << 31) != 0 and 'N ' in err()
    assert pr(pix=None) != 0 and 'null pointer' in err()
    assert pr(pix=p + 2) != 0 and 'aligned' in err()
    assert pr(idx=p + 4) != 0 and 'aligned' in err()
    names = ('rays_o', 'rays_d', 't_exp', 't_med', 'valid', 'surface', 'alpha', 'woff', 'pix2ray', 'N', 'H', 'W', 'edge', 'M',
             'bgcolor', 'lohi', 'ambient', 'albedo', 'truth8', 'status', 'normal', 'nvalid', 'normal8', 'depth8', 'shaded8',
             'offset8')
    base = dict(surface=0, N=4, H=2, W=2, edge=0.05, ambient=0.25, albedo=0.8, truth8=None, status=None)
    gm = lambda **k: lib.hnrf_geometry_maps(*[k[a] if a in k else base.get(a, p) for a in names], None)
    assert gm(surface=2) != 0 and 'surface 2' in err()
    assert gm(edge=float('nan')) != 0 and 'edge' in err()
    assert gm(edge=-1.0) != 0 and 'edge' in err()
    assert gm(H=0) != 0 and 'H 0' in err()
    assert gm(surface=1, t_med=None) != 0 and 't_med' in err()
    assert gm(M=None) != 0 and 'normal8 needs M' in err()
    assert gm(lohi=None) != 0 and 'depth8 needs lohi' in err()
    assert gm(alpha=None) != 0 and 'shaded8 needs alpha' in err()
    assert gm(woff=None) != 0 and 'offset8 needs woff' in err()
    assert gm(pix2ray=p + 1) != 0 and 'aligned' in err()


def test_config_refuses_what_the_lean_form_cannot_give():
    from humannerf_amd.config import check_amd_options
    check_amd_options({'maps': ['depth', 'normal', 'shaded', 'offset'], 'maps_surface': 'median'})
    check_amd_options({'maps': ['depth', 'normal', 'shaded'], 'diagnostics': False})
    with pytest.raises(ValueError, match='cfg.amd.maps'):
        check_amd_options({'maps': ['depth', 'curvature']})
    with pytest.raises(ValueError, match='cfg.amd.maps'):
        check_amd_options({'maps': 'depth'})
    with pytest.raises(ValueError, match='maps_surface'):
        check_amd_options({'maps_surface': 'mode'})
    for bad in ({'maps': ['offset']}, {'maps': ['depth'], 'maps_surface': 'median'}):
        with pytest.raises(ValueError) as e:
            check_amd_options(dict(bad, diagnostics=False))
        assert 'cfg.amd.maps' in str(e.value) and 'cfg.amd.maps_surface' in str(e.value) and 'diagnostics' in str(e.value)
    with pytest.raises(ValueError, match='perturb'):
        from humannerf_amd.config import cfg
        old = cfg.perturb
        cfg.perturb = 1.0
        try:
            geo.frame_maps({}, {}, 2, 2, None)
        finally:
            cfg.perturb = old


def test_select_panels_appends_the_maps_last():
    from humannerf_amd import render
    from humannerf_amd.config import cfg
    a, b, c = (np.full((2, 2, 3), v, np.uint8) for v in (1, 2, 3))
    old = cfg.get('show_truth', False), cfg.get('show_alpha', False)
    cfg.show_truth, cfg.show_alpha = True, True
    try:
        assert [int(p[0, 0, 0]) for p in render.select_panels(a, b, c)] == [1, 3, 2]
        got = render.select_panels(a, b, c, maps={'depth': a * 7, 'normal': a * 9})
        assert [int(p[0, 0, 0]) for p in got] == [1, 3, 2, 7, 9]
        assert len(render.select_panels(a, b, c, maps=None)) == 3 and len(render.select_panels(a, b, c, maps={})) == 3
    finally:
        cfg.show_truth, cfg.show_alpha = old
