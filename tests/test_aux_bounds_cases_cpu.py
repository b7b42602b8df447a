"""The cases of tests/aux_bounds_cases.py through the numpy twins: every case runs on the host route, and the conditions
that keep tests/test_gpu_aux_buffer_bounds.py from passing vacuously are asserted here on the twin alone -- a mesh has
vertices and faces, a compaction keeps some rows and drops some, a distance has matched and unmatched points, a
rasterised triangle covers some pixels and leaves some, the noise image fills more than half of the stream's worst
case, and the cases meant to raise a status word raise it.  No GPU."""
import numpy as np
import pytest

from humannerf_amd import cloud, geometry as geo, imageproc as ip, mesh, raster, render, skin, video
from tests import aux_bounds_cases as ac


# ---------------------------------------------------------------------------------------------- image pre-processing
@pytest.mark.parametrize('name', list(ac.UNDISTORT_CASES))
def test_undistort_cases_tap_outside_the_image(name):
    c = ac.undistort_case(name)
    H, W, C = c['img'].shape
    ix, iy, _, _ = ip.undistort_maps(c['K'], c['D'], H, W)
    gone = (ix >= W) | (ix + 1 < 0) | (iy >= H) | (iy + 1 < 0)                     # all four taps outside: constant 0
    partly = ~gone & ((ix < 0) | (ix + 1 >= W) | (iy < 0) | (iy + 1 >= H))
    inside = (ix >= 0) & (ix + 1 < W) & (iy >= 0) & (iy + 1 < H)
    assert gone.any() and (partly.any() or inside.any())
    out = ip.undistort_u8(c['img'], c['K'], c['D'])
    assert out.shape == c['img'].shape and (out[gone] == 0).all() and (out != 0).any()    # (the image itself has no zero)
    if name == '64x80x1':
        assert c['n_stripes'] == 2 and 0 < H - c['rows'] < c['rows']                   # a ragged last stripe
    else:
        assert c['n_stripes'] == 1 and c['rows'] == H


@pytest.mark.parametrize('scale', ac.COMPOSITE_SCALES)
def test_composite_windows_touch_all_four_borders(scale):
    c = ac.composite_case(scale)
    img = ip.load_step(c['orig'], c['alpha'], c['bg'], scale=scale)[0]
    assert img.shape[:2] == (c['Hd'], c['Wd']) and len(c['wins']) == 6
    x0, y0 = c['wins'][:, 0], c['wins'][:, 1]
    assert x0.min() == 0 and y0.min() == 0 and (x0 + 4).max() == c['Wd'] and (y0 + 4).max() == c['Hd']
    whole = ac.composite_case(scale, whole=True)
    assert (whole['ph'], whole['pw']) == (c['Hd'], c['Wd']) and len(whole['wins']) == 1
    if scale != 1.0:                                                                   # taps leave the source on every side
        xo, _, yo, _ = c['tables']
        assert xo.min() - 3 < 0 and xo.max() + 4 > ac.COMPOSITE_SRC[1] - 1 and yo.min() - 3 < 0 and yo.max() + 4 > ac.COMPOSITE_SRC[0] - 1


@pytest.mark.parametrize('case', ac.MASK_CASES, ids=str)
def test_mask_cases_take_the_stated_mode(case):
    c = ac.mask_case(*case)
    out = ip.resize_f64(c['alpha'] / 255., c['scale'], 'linear')[:, :, ac.MASK_CHANNEL]
    assert out.shape == (c['Hd'], c['Wd']) and (c['tables'] is None) == (c['mode'] == 2)
    assert {m for _, _, m in ac.MASK_CASES} == {1, 2} and any(h % 2 and w % 2 for (h, w), _, _ in ac.MASK_CASES)


# ------------------------------------------------------------------------------------------------- mesh extraction
@pytest.mark.parametrize('name', ac.MESH_CASES)
def test_mesh_cases_have_a_surface(name):
    c = ac.mesh_case(name)
    v, f = mesh.mesh_from_density_host(c['d'], c['bmin'], c['bmax'], c['level'])
    if c['empty']:
        assert len(v) == 0 and len(f) == 0 and (c['d'] <= c['level']).all()
        return
    assert len(v) > 1 and len(f) > 1 and f.max() == len(v) - 1
    on_boundary = (np.abs(v) == 1.0).any()
    assert on_boundary == name.startswith('open')


# -------------------------------------------------------------------------------------- skinning and field normals
@pytest.mark.parametrize('extra', ac.SKIN_EXTRA)
@pytest.mark.parametrize('shape', ac.SKIN_SHAPES, ids=str)
def test_skin_cases_on_the_host(shape, extra):
    V, B, G = shape
    c = ac.skin_case(V, B, G, extra)
    assert c['vol'].shape[0] == B + extra and c['mats'].shape[0] == B
    for K in ac.SKIN_KS:
        j, w, kept = skin.skin_weights_host(c['verts'], c['vol'], c['bmin'], c['scale'], k=K, n_bones=B)
        assert j.shape == (V, K) and j.dtype == np.uint8 and (j < B).all()
        jl, wl = ac.lbs_inputs(c, K)
        out = skin.skin_lbs_host(c['verts'], jl, wl, c['mats'])
        assert out.shape == (V, 3)
        if V:
            assert (jl >= B).any()                                            # the slot that must be skipped
        if V > 4:
            assert kept[1] == 0 and kept[2] == 0 and kept[0] > 0              # far outside / NaN: nothing; the corner: a weight
            assert (j[1] == 0).all() and w[2, 0] == 1
    n = geo.field_normals_host(c['verts'], c['g'], c['sigma'], c['vol'], c['bmin'], c['scale'], n_bones=min(B, 32))
    assert n.shape == (V, 3) and np.isfinite(n).all()


# ------------------------------------------------------------------------------------------------------- rasteriser
@pytest.mark.parametrize('size', ac.RASTER_SIZES, ids=str)
@pytest.mark.parametrize('scene', ac.RASTER_SCENES)
def test_raster_cases_cover_some_pixels_and_leave_some(scene, size):
    H, W = size
    c = ac.raster_case(scene, H, W)
    for shade, colors in (('color', c['colors']), ('normal', None)):
        out = raster.rasterize_host(c['verts'], c['faces'], colors, c['K'], c['E'], H, W, bgcolor=c['bg'], shade=shade)
        tri = out['tri_id']
        if scene == 'hang':
            assert set(np.unique(tri)) <= {-1, 0} and (tri == 0).any()        # the two bad faces are dropped
            if H * W > 1:
                assert (tri == -1).any() and tri[0, 0] == -1 and tri[H - 1, 0] == 0 and tri[H - 1, W - 1] == 0
        elif scene == 'cover':
            assert set(np.unique(tri)) <= {0, 1} and (tri == 1).any() and ((tri == 0).any() or H * W == 1)
        else:
            assert (tri == -1).all() and (out['alpha'] == 0).all()


# --------------------------------------------------------------------------------------------------- image metrics
@pytest.mark.parametrize('mask_kind', ac.METRIC_MASKS)
@pytest.mark.parametrize('size', ac.METRIC_SIZES, ids=str)
@pytest.mark.parametrize('n_img', [1, 3])
def test_metric_cases_hit_the_nan_rules(n_img, size, mask_kind):
    H, W = size
    a, b, m = ac.metrics_case(n_img, H, W, mask_kind)
    out = render.metrics_u8(a, b, m)
    assert out.shape == (n_img, 2)
    kinds = ac.METRIC_MASKS[1:]
    for i in range(n_img):
        kind = 'none' if m is None else kinds[(kinds.index(mask_kind) + i) % 3]
        if kind == 'empty':
            assert np.isnan(out[i]).all()
        elif kind == 'narrow':
            assert np.isfinite(out[i, 0]) and np.isnan(out[i, 1])
        elif kind == 'L':
            ys, xs = np.nonzero(m[i])
            box = (ys.max() - ys.min() + 1) * (xs.max() - xs.min() + 1)
            assert np.isfinite(out[i, 0]) and (box > m[i].astype(bool).sum() or min(H, W) < 8)
            assert np.isfinite(out[i, 1]) == (min(ys.max() - ys.min(), xs.max() - xs.min()) + 1 >= 7)
        else:
            assert np.isfinite(out[i]).all()


# ----------------------------------------------------------------------------------------------------------- clouds
def test_cloud_cases_on_the_twin():
    for R in (1, 5):                                                          # (the twin takes no R = 0; the entry launches nothing)
        for S in (1, 63, 65):
            for B in (1, 24, 32):
                wxyz, wmax, lbs = cloud.twin_surface_points(*ac.rays_case(R, S, B))
                assert wxyz.shape == (R, 3) and lbs.shape == (R,) and (lbs < B).all()
    for Na, Nb in ac.NN_SHAPES:
        idx, d2 = cloud.twin_nn(*ac.nn_case(Na, Nb))
        assert idx.shape == (Na,) and ((idx == -1).all() if Nb == 0 else (idx >= 0).all())


def test_distance_case_has_matched_and_unmatched_points():
    c = ac.pairs_case()
    D, match = ac.pairs_twin(c)
    assert (match[0] >= 0).all() and D[0] == 0.0                              # (2, 2): every point finds itself
    assert (match[1] >= 0).sum() == 1 and D[1] > 0                            # (2, 1): one partner among 300
    assert (match[2:] == -1).all() and (D[2:] == 0).all()                     # no such frame; a frame outside total
    assert c['offsets'][4] > c['total'] and c['pairs'][2, 1] >= c['F']
    # tau decides: the 300 points against themselves shifted by half of tau match in part
    other = dict(c['frames'][2], xyz=(c['frames'][2]['xyz'] + np.float32(0.5 * c['tau'])))
    m, _, _ = cloud.twin_pairs(c['frames'][2], cloud.sort_frame(other['xyz'], other['rgb'], c['axis']), c['tau'], c['axis'])
    assert 0 < (m >= 0).sum() < 300


# ------------------------------------------------------------------------------------------------------------ JPEG
def test_jpeg_noise_gives_long_mcus():
    """How long an MCU the 16 x 16 noise image gives at quality 100.  hnrf_jpeg_max_bytes (3522 for one MCU) is out of
    any picture's reach: it allows every coefficient a 16-bit code, 10 amplitude bits and a stuffed byte each (2496),
    while the 64 coefficients of a block share the energy of its 64 samples (|s| <= 128: Parseval), so at most a few
    reach category 10 and a block of 64 equal coefficients of 128 takes 18 bits each: 864 bytes for the six blocks.  A
    stream above half of hnrf_jpeg_max_bytes (1761 bytes) would need an MCU of 1146.  So the condition is stated against
    that dense bound: the MCU takes more than half of 864 bytes, which is seven passes of the 64-lane stuffing loop."""
    img = ac.jpeg_image(16, 16)
    n = len(video.jpeg_encode_numpy(img, 100))
    mcu = n - len(video.jpeg_header(16, 16, 100)) - 2
    dense = 6 * 64 * 18 // 8
    print('16 x 16 noise at q = 100: %d bytes, MCU %d, dense bound %d, hnrf_jpeg_max_bytes %d'
          % (n, mcu, dense, video.HEADER_MAX + video.SLOT_BYTES + 2))
    assert mcu > dense // 2 >= 6 * 64, (n, mcu)
    assert len(video.jpeg_encode_numpy(img, 1)) - 615 < mcu // 8             # quality 1: the short end
    for H, W in ac.JPEG_SIZES:
        for pad in ac.JPEG_PADS:
            buf, stride = ac.jpeg_tight(ac.jpeg_image(H, W), pad)
            assert buf.size == (H - 1) * stride + 3 * W and stride == 3 * W + pad
            rows = np.stack([buf[y * stride:y * stride + 3 * W] for y in range(H)]).reshape(H, W, 3)
            assert np.array_equal(rows, ac.jpeg_image(H, W))


# --------------------------------------------------------------------------------------------------- segmentation
@pytest.mark.parametrize('n_parts', list(ac.SEG_PARTS))
@pytest.mark.parametrize('radius', ac.SEG_RADII)
def test_segment_cases_keep_some_rows_and_drop_some(radius, n_parts):
    c = ac.segment_case()
    assert c['total'] == c['rec'].shape[0] == c['offsets'][-1] + 1           # one row outside every frame
    shared = (c['frames'][0][:, 7] == 3) & (c['frames'][0][:, 8] == 4)
    assert shared.sum() >= 2
    for weighted in (False, True):
        member, seg, src = ac.segment_twin(c, n_parts, radius, weighted)
        assert member.shape == (c['total'],) and member[-1] == 0 and seg.shape == (n_parts * c['F'] + 1,)
        per_part = np.diff(seg).reshape(n_parts, c['F']).sum(1)
        kept_and_dropped = (per_part > 0) & (per_part < c['total'] - 1)
        if weighted or radius == 1:              # (radius 33 covers the 7 x 30 image: without weights every part keeps all)
            assert kept_and_dropped.sum() >= min(2, n_parts), per_part
        else:
            assert (per_part == c['total'] - 1).all()
        assert seg[-1] == src.size > 0
    plain = ac.segment_twin(c, n_parts, radius, False)[2]
    assert src.size < plain.size and 10 in plain and 11 in plain and 10 not in src      # the NaN weight is dropped
    with pytest.raises(ValueError, match='outside'):                         # status bit 2 on the device
        ac.segment_twin(ac.segment_case(bad=True), n_parts, radius, False)


# --------------------------------------------------------------------------------------------------- geometry maps
def test_geometry_cases_on_the_twin():
    from tests import geometry_cases as gc
    for R in ac.SURFACE_R:
        for S in ac.SURFACE_S:
            near, far, alpha, depth, w, off = gc.surface_inputs(R, S, seed=R * 100 + S)
            full = geo.ray_surface_host(near, far, alpha, depth, w, off, want_median=True, want_woff=True)
            assert full['t_exp'].shape == (R,) and full['woff'].shape == (R, 3)
    for H, W in ac.MAP_SIZES:
        c = ac.maps_case(H, W)
        p2r, st = geo.pixel_rays_host(c['ray_index'], H, W)
        assert st == 0
        if H * W > 1:
            assert p2r[c['ray_index'][0]] == c['N'] - 1                       # two rays on one pixel: the highest wins
        out = geo.maps_host(c['o'], c['d'], c['surf'], p2r, H, W, alpha=c['alpha'], M=c['M'], bgcolor=c['bg'], lohi=c['lohi'],
                            truth8=c['truth'])
        assert set(out) == set(geo.OUTPUTS)
        assert geo.pixel_rays_host(ac.maps_case(H, W, bad_index=True)['ray_index'], H, W) == (None, 1)


# ----------------------------------------------------------------------------------------- density-gradient normals
@pytest.mark.parametrize('kind', ac.NORMALS_COUNTS)
@pytest.mark.parametrize('shape', ac.NORMALS_SHAPES, ids=str)
def test_ray_normals_cases_on_the_twin(shape, kind):
    R, S, B = shape
    c = ac.ray_normals_case(R, S, B, kind)
    assert c['idx'].shape == (c['n_max'],) and c['g'].shape == (c['n_max'], 3) and c['n_max'] >= 1
    assert ((c['idx'] < 0) | (c['idx'] >= R * S)).any()
    n, ok = ac.ray_normals_twin(c)
    assert n.shape == (R, 3) and ok.shape == (R,)
    if kind == 'zero':
        assert not ok.any() and (n == 0).all()
    assert {'over': c['count'][0] > c['n_max'], 'equal': c['count'][0] == c['n_max'], 'zero': c['count'][0] == 0}[kind]


def test_some_ray_normals_case_has_valid_and_invalid_rays():
    oks = np.concatenate([ac.ray_normals_twin(ac.ray_normals_case(R, S, B, 'equal'))[1] for R, S, B in ac.NORMALS_SHAPES])
    assert oks.any() and not oks.all()
