"""The rasteriser's host route (humannerf_amd.raster.rasterize_host) against properties that follow from its stated
conventions -- watertight shared edges, even coverage of a closed surface, the analytic sphere, order independence,
perspective-correct colours, dropped triangles -- and the host-side argument checks of hnrf_raster_mesh.  No GPU.
The case builders here are shared with tests/test_gpu_raster.py, which holds the device route to the same pictures."""
import numpy as np
import pytest

from humannerf_amd import mesh, raster, scene

EYE_K, EYE_E = np.eye(3, dtype=np.float32), np.eye(4, dtype=np.float32)
LOOKAT = np.array([0.0, -0.25, 0.0])                   # of scene.tpose_camera
SPHERE_N, SPHERE_R = 48, 0.8
STEP = 2.0 / (SPHERE_N - 1)                            # lattice step h


# ------------------------------------------------------------------------------------------------------- case builders
def polygons(n=120, seed=0):
    """Convex polygons with 3-8 vertices on a circle of 6-26 px radius around a centre near (32, 32), everything on
    the 1/256 grid, adjacent directions at least 0.15 rad apart and less than pi - 0.15 (the centre is inside).  Every
    fourth has an integer centre and radius and its first direction along +x: centre and first vertex are sample
    points.  Yields (centre (2,), vertices (nv, 2)) in float64, exactly representable in float32."""
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        nv = int(rs.randint(3, 9))
        gaps = 0.15 + rs.dirichlet(np.ones(nv)) * (2 * np.pi - 0.15 * nv)
        if gaps.max() >= np.pi - 0.15:
            continue
        on_samples = len(out) % 4 == 0
        if on_samples:
            c = np.array([float(rs.randint(30, 35)), float(rs.randint(30, 35))])
            r, th0 = float(rs.randint(6, 27)), 0.0
        else:
            c = np.rint(rs.uniform(30.0, 34.0, 2) * 256) / 256
            r, th0 = rs.uniform(6.0, 26.0), rs.uniform(0, 2 * np.pi)
        th = th0 + np.concatenate([[0.0], np.cumsum(gaps[:-1])])
        v = np.rint((c + r * np.stack([np.cos(th), np.sin(th)], 1)) * 256) / 256
        out.append((c, v))
    return out


def polygon_meshes(c, v):
    """(verts (nv + 1, 3) at z = 1 with the centre last, {name: faces}): the fan around the centre, the fan from
    boundary vertex 0, and the first with every winding reversed."""
    nv = len(v)
    verts = np.concatenate([np.concatenate([v, c[None]], 0), np.ones((nv + 1, 1))], 1).astype(np.float32)
    centre = np.array([[nv, i, (i + 1) % nv] for i in range(nv)], dtype=np.int32)
    boundary = np.array([[0, i, i + 1] for i in range(1, nv - 1)], dtype=np.int32)
    return verts, {'centre': centre, 'boundary': boundary, 'reversed': np.ascontiguousarray(centre[:, ::-1])}


def field_mesh(N, f, lo=-1.0, hi=1.0):
    """mesh_from_density_host of f(x, y, z) at level 0 on an N^3 lattice over [lo, hi]^3, moved to the look-at point."""
    ax = mesh.lattice_axes([lo] * 3, [hi] * 3, N)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    d = f(x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)).astype(np.float32)
    verts, faces = mesh.mesh_from_density_host(d, [lo] * 3, [hi] * 3, 0.0)
    return (verts + LOOKAT.astype(np.float32)).astype(np.float32), faces


def sphere_mesh():
    return field_mesh(SPHERE_N, lambda x, y, z: SPHERE_R - np.sqrt(x * x + y * y + z * z))


def tpose_camera(size):
    """scene.tpose_camera framed for a size x size image (focal 1250 at 512)."""
    return scene.tpose_camera(np.array([size, size], dtype=np.float32), focal=1250.0 * size / 512.0)


def vertex_colors(verts, seed=1):
    return np.random.RandomState(seed).uniform(0, 1, verts.shape).astype(np.float32)


def soup(n=20000, size=256, seed=5):
    """Triangle soup for the identity camera: sizes log-uniform from 0.05 to 300 px, a tenth of the triangles centred
    up to 200 px outside the image, depths 0.5-8 per vertex, 2 % with a vertex behind the camera."""
    rs = np.random.RandomState(seed)
    s = np.exp(rs.uniform(np.log(0.05), np.log(300.0), n))
    c = rs.uniform(0, size, (n, 2))
    off = rs.rand(n) < 0.1
    c[off] = rs.uniform(-200, size + 200, (int(off.sum()), 2))
    uv = c[:, None, :] + rs.uniform(-0.5, 0.5, (n, 3, 2)) * s[:, None, None]
    z = rs.uniform(0.5, 8.0, (n, 3))
    z[rs.rand(n) < 0.02, 0] = -1.0
    verts = np.concatenate([uv * z[..., None], z[..., None]], -1).reshape(-1, 3).astype(np.float32)
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def pixel_rays(K, E, H, W):
    o, d = scene.get_rays_from_KRT(H, W, K.astype(np.float64), E[:3, :3].astype(np.float64), E[:3, 3].astype(np.float64))
    return np.asarray(o, np.float64), np.asarray(d, np.float64)


def hit_sphere(o, d, r, c=LOOKAT):
    """(hits (H, W) bool, t of the near intersection) of the rays o + t d with the sphere |x - c| = r."""
    oc = o - c
    a, b, cc = (d * d).sum(-1), (oc * d).sum(-1), (oc * oc).sum(-1) - r * r
    disc = b * b - a * cc
    return disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a


# -------------------------------------------------------------------------------------------------------------- tests
def test_shared_edges_are_covered_exactly_once():
    H = W = 64
    polys = polygons(120)
    assert len(polys) >= 100
    on_grid = 0
    for c, v in polys:
        verts, fans = polygon_meshes(c, v)
        on_grid += int(np.all(c == np.rint(c)))
        covered = {}
        for name, faces in fans.items():
            count = np.zeros((H, W))
            for f in faces:
                count += raster.rasterize_host(verts, f[None], None, EYE_K, EYE_E, H, W, shade='normal')['alpha']
            assert count.max() <= 1, name
            whole = raster.rasterize_host(verts, faces, None, EYE_K, EYE_E, H, W, shade='normal')['alpha']
            assert np.array_equal(whole, count)
            covered[name] = count > 0
        assert np.array_equal(covered['centre'], covered['boundary'])
        assert np.array_equal(covered['centre'], covered['reversed'])
        # (the polygon is really drawn: its sample count is its area up to the samples along the perimeter)
        x, y = v[:, 0], v[:, 1]
        area = 0.5 * abs(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
        perimeter = np.sum(np.hypot(x - np.roll(x, -1), y - np.roll(y, -1)))
        assert abs(covered['centre'].sum() - area) <= perimeter
    assert on_grid >= 25                                   # centres and first vertices exactly on sample points


@pytest.fixture(scope='module')
def sphere():
    verts, faces = sphere_mesh()
    K, E = tpose_camera(128)
    out = {cull: raster.rasterize_host(verts, faces, None, K, E, 128, 128, cull=cull, shade='normal')
           for cull in ('none', 'back', 'front')}
    return verts, faces, K, E, out


def test_closed_surface_is_covered_evenly(sphere):
    verts, faces, K, E, out = sphere
    back, front = out['back'], out['front']
    assert faces.shape[0] > 10000 and back['alpha'].sum() > 4000
    assert np.array_equal(back['alpha'], front['alpha'])
    assert np.array_equal(back['alpha'], out['none']['alpha'])
    cov = back['alpha'] > 0
    assert np.all(back['depth'][cov] < front['depth'][cov])            # culling back faces leaves the near side
    assert np.array_equal(out['none']['tri_id'], back['tri_id']) and np.array_equal(out['none']['depth'], back['depth'])


def test_geometry_matches_the_analytic_sphere(sphere):
    verts, faces, K, E, out = sphere
    back = out['back']
    cov = back['alpha'] > 0
    o, d = pixel_rays(K, E, 128, 128)
    slack = np.sqrt(3.0) * STEP
    inner, _ = hit_sphere(o, d, SPHERE_R - slack)
    outer, _ = hit_sphere(o, d, SPHERE_R + slack)
    assert inner.sum() > 4000
    assert np.all(cov[inner]) and np.all(outer[cov])
    p = o + d * back['depth'].astype(np.float64)[..., None]
    err = np.abs(np.linalg.norm(p - LOOKAT, axis=-1) - SPHERE_R)[cov]
    bound = 2 * 3 * STEP ** 2 / (8 * (SPHERE_R - slack))
    print('sphere depth: max | |p - c| - 0.8 | = %.3e (bound %.3e)' % (err.max(), bound))
    assert 1.8e-3 < bound < 1.9e-3
    assert err.max() <= bound


def test_normal_shade_on_the_sphere(sphere):
    verts, faces, K, E, out = sphere
    back = out['back']
    o, d = pixel_rays(K, E, 128, 128)
    away, _ = hit_sphere(o, d, SPHERE_R - 4 * STEP)
    _, t = hit_sphere(o, d, SPHERE_R)
    sel = away & (back['alpha'] > 0)
    assert sel.sum() > 3000
    n = (o + d * t[..., None] - LOOKAT) / SPHERE_R
    want = 0.5 + 0.5 * n @ E[:3, :3].astype(np.float64).T
    dev = np.abs(back['rgb'].astype(np.float64) - want)[sel]
    print('sphere normals: max deviation %.4f (bound 0.05)' % dev.max())
    assert dev.max() <= 0.05
    assert np.all(back['rgb'][~(back['alpha'] > 0)] == 0)              # background colour elsewhere


def test_order_ties_and_exact_depth():
    H = W = 32
    near = np.array([[4, 4, 1], [28, 6, 1], [10, 27, 1]], np.float64) * [2, 2, 2]          # z = 2: u, v = 4..28
    far = np.array([[2, 10, 1], [30, 12, 1], [14, 30, 1]], np.float64) * [3, 3, 3]
    verts = np.concatenate([near, far]).astype(np.float32)
    col = vertex_colors(verts)
    a = raster.rasterize_host(verts, np.array([[0, 1, 2], [3, 4, 5]], np.int32), col, EYE_K, EYE_E, H, W)
    b = raster.rasterize_host(verts, np.array([[3, 4, 5], [0, 1, 2]], np.int32), col, EYE_K, EYE_E, H, W)
    both = (a['tri_id'] >= 0)
    only_near = raster.rasterize_host(verts, np.array([[0, 1, 2]], np.int32), col, EYE_K, EYE_E, H, W)
    only_far = raster.rasterize_host(verts, np.array([[3, 4, 5]], np.int32), col, EYE_K, EYE_E, H, W)
    overlap = (only_near['alpha'] > 0) & (only_far['alpha'] > 0)
    assert overlap.sum() > 50 and np.all(a['tri_id'][overlap] == 0) and np.all(b['tri_id'][overlap] == 1)
    for k in ('rgb', 'alpha', 'depth'):
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(np.where(both, 1 - a['tri_id'], -1), b['tri_id'])
    # a fronto-parallel triangle at z = 2 has depth exactly 2
    assert np.all(only_near['depth'][only_near['alpha'] > 0] == 2.0) and np.all(only_near['depth'][only_near['alpha'] == 0] == 0)
    # coincident triangles: the lower index wins, and a permutation of faces shows only through tri_id
    tri = np.array([[0, 1, 2], [3, 4, 5], [1, 2, 0], [0, 1, 2]], np.int32)
    c = raster.rasterize_host(verts, tri, col, EYE_K, EYE_E, H, W)
    assert np.all(c['tri_id'][only_near['alpha'] > 0] == 0)
    perm = np.array([3, 1, 0, 2])                                       # new face k = old face perm[k]
    p = raster.rasterize_host(verts, tri[perm], col, EYE_K, EYE_E, H, W)
    assert np.all(p['tri_id'][only_near['alpha'] > 0] == 0)             # (old 3 = the same triangle, now first)
    for k in ('rgb', 'alpha', 'depth'):
        assert np.array_equal(c[k], p[k])
    far_only = (c['tri_id'] == 1)
    assert far_only.sum() > 0 and np.all(p['tri_id'][far_only] == 1)


def tilted_triangle():
    """One triangle ~200 px across with depths 1, 4, 2 whose corners project exactly onto pixel centres, coloured by an
    affine function of the world position.  Returns (verts, colors, uvz, colour function)."""
    uvz = np.array([[10.0, 20.0, 1.0], [210.0, 40.0, 4.0], [60.0, 215.0, 2.0]])
    verts = np.stack([uvz[:, 0] * uvz[:, 2], uvz[:, 1] * uvz[:, 2], uvz[:, 2]], 1)
    fn = lambda p: np.stack([p[..., 0] / 1000.0 + 0.05, p[..., 1] / 500.0 + 0.05, (p[..., 2] - 1.0) * 0.3 + 0.05], -1)
    return verts.astype(np.float32), fn(verts).astype(np.float32), uvz, fn


def test_colour_is_perspective_correct():
    H = W = 224
    verts, col, uvz, fn = tilted_triangle()
    assert np.array_equal(verts.astype(np.float64)[:, 0], uvz[:, 0] * uvz[:, 2]) and col.min() >= 0 and col.max() <= 1
    out = raster.rasterize_host(verts, np.array([[0, 1, 2]], np.int32), col, EYE_K, EYE_E, H, W)
    cov = out['alpha'] > 0
    assert cov.sum() > 15000
    j, i = np.nonzero(cov)
    d = np.stack([i, j, np.ones_like(i)], 1).astype(np.float64)         # the identity camera's pixel rays
    p0, p1, p2 = verts.astype(np.float64)
    n = np.cross(p1 - p0, p2 - p0)
    hit = d * ((n @ p0) / (d @ n))[:, None]
    err = np.abs(out['rgb'][cov].astype(np.float64) - fn(hit))
    print('perspective colour: max error %.3e (bound 1e-5)' % err.max())
    assert err.max() <= 1e-5
    assert np.abs(out['depth'][cov] - hit[:, 2]).max() <= 1e-5
    # screen-space-affine interpolation of the same colours is far off: the test can tell the two apart
    T = np.array([[uvz[1, 0] - uvz[0, 0], uvz[2, 0] - uvz[0, 0]], [uvz[1, 1] - uvz[0, 1], uvz[2, 1] - uvz[0, 1]]])
    b12 = np.linalg.solve(T, np.stack([i - uvz[0, 0], j - uvz[0, 1]]))
    affine = col[0] + b12[0][:, None] * (col[1] - col[0]).astype(np.float64) + b12[1][:, None] * (col[2] - col[0]).astype(np.float64)
    assert np.abs(affine - fn(hit)).max() > 1e-2


def test_dropped_triangles_render_as_absent():
    H = W = 32
    good = np.array([[3, 3, 1], [29, 5, 1], [8, 28, 1]], np.float32)
    extra = {
        'behind z_near': np.array([[5, 5, 1], [25, 5, 1], [15, 25, 1e-4]], np.float32),
        'behind the camera': np.array([[5, 5, 1], [25, 5, 1], [15, 25, -1]], np.float32),
        'outside the guard band': np.array([[5, 5, 1], [25, 5, 1], [2.0e4, 25, 1]], np.float32),
        'nan': np.array([[5, 5, 1], [25, np.nan, 1], [15, 25, 1]], np.float32),
        'inf': np.array([[5, 5, 1], [np.inf, 5, 1], [15, 25, 1]], np.float32),
        'zero area': np.array([[5, 5, 1], [10, 10, 1], [20, 20, 1]], np.float32),
    }
    col3 = vertex_colors(good)
    alone = raster.rasterize_host(good, np.array([[0, 1, 2]], np.int32), col3, EYE_K, EYE_E, H, W, bgcolor=(0.2, 0.4, 0.6))
    assert alone['alpha'].sum() > 200
    assert np.all(alone['rgb'][alone['alpha'] == 0] == np.array([0.2, 0.4, 0.6], np.float32))
    for name, bad in extra.items():
        bad = bad.copy()
        bad[:, :2] *= bad[:, 2:3]                                       # (u, v, z) -> world
        bad[:, 2] *= 0.5 if name not in ('behind z_near', 'behind the camera') else 1.0   # nearer than `good`
        bad[:, :2] *= 0.5 if name not in ('behind z_near', 'behind the camera') else 1.0
        verts = np.concatenate([good, bad])
        col = np.concatenate([col3, vertex_colors(bad, 2)])
        for faces, own in (([[0, 1, 2], [3, 4, 5]], 0), ([[3, 4, 5], [0, 1, 2]], 1)):
            out = raster.rasterize_host(verts, np.array(faces, np.int32), col, EYE_K, EYE_E, H, W, bgcolor=(0.2, 0.4, 0.6))
            for k in ('rgb', 'alpha', 'depth'):
                assert np.array_equal(out[k], alone[k]), (name, k)
            assert np.array_equal(out['tri_id'], np.where(alone['tri_id'] >= 0, own, -1)), name
    # the nearer copies would have shown had they not been dropped
    shown = np.concatenate([good, good * np.float32(0.5)])
    out = raster.rasterize_host(shown, np.array([[0, 1, 2], [3, 4, 5]], np.int32), np.concatenate([col3, col3]), EYE_K,
                                EYE_E, H, W)
    assert np.all(out['tri_id'][alone['alpha'] > 0] == 1)
    # face indices outside [0, V)
    for bad_face in ([0, 1, 3], [0, -1, 2], [2 ** 31 - 1, 1, 2]):
        out = raster.rasterize_host(good, np.array([bad_face, [0, 1, 2]], np.int32), col3, EYE_K, EYE_E, H, W,
                                    bgcolor=(0.2, 0.4, 0.6))
        assert np.array_equal(out['rgb'], alone['rgb']) and np.array_equal(out['tri_id'], np.where(alone['tri_id'] >= 0, 1, -1))
    # nothing to draw
    for v, f in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), (good, np.zeros((0, 3), np.int32)),
                 (np.zeros((0, 3), np.float32), np.array([[0, 1, 2]], np.int32))):
        out = raster.rasterize_host(v, f, v, EYE_K, EYE_E, H, W, bgcolor=(0.2, 0.4, 0.6))
        assert np.all(out['tri_id'] == -1) and np.all(out['alpha'] == 0) and np.all(out['depth'] == 0)
        assert np.all(out['rgb'] == np.array([0.2, 0.4, 0.6], np.float32))


def test_mirrored_camera_flips_the_facing():
    """det(K R) < 0 (a mirrored camera): what is front-facing swaps; the picture mirrors."""
    verts, faces = field_mesh(24, lambda x, y, z: 0.6 - np.sqrt(x * x + y * y + z * z))
    K, E = tpose_camera(64)
    Km = K.copy()
    Km[0, 0] = -K[0, 0]
    Km[0, 2] = 63.0 - K[0, 2]                                           # u -> 63 - u
    assert not raster.camera_flips(K, E[:3, :3]) and raster.camera_flips(Km, E[:3, :3])
    a = raster.rasterize_host(verts, faces, None, K, E, 64, 64, cull='back', shade='normal')
    b = raster.rasterize_host(verts, faces, None, Km, E, 64, 64, cull='back', shade='normal')
    f = raster.rasterize_host(verts, faces, None, K, E, 64, 64, cull='front', shade='normal')
    cov = a['alpha'] > 0
    assert cov.sum() > 500
    assert np.all(a['depth'][cov] < f['depth'][cov])
    # the mirrored picture shows the near side too (the fill rule may move silhouette samples: compare the interior)
    inner = cov & np.roll(cov, 1, 1) & np.roll(cov, -1, 1) & np.roll(cov, 1, 0) & np.roll(cov, -1, 0)
    bm = {k: v[:, ::-1] for k, v in b.items()}
    assert np.all(bm['alpha'][inner] > 0)
    assert np.abs(bm['depth'][inner] - a['depth'][inner]).max() < 0.05


def test_image_need_not_be_square():
    """A smaller image with the same camera is the top-left corner of the larger one."""
    verts, faces = field_mesh(32, lambda x, y, z: 0.04 - (np.sqrt(x * x + y * y) - 0.5) ** 2 - z * z)
    col = vertex_colors(verts)
    K, E = tpose_camera(160)
    full = raster.rasterize_host(verts, faces, col, K, E, 160, 160, cull='back')
    assert (full['tri_id'] >= 0).sum() > 2000
    for H, W in ((96, 160), (160, 72), (64, 100)):
        part = raster.rasterize_host(verts, faces, col, K, E, H, W, cull='back')
        assert (part['tri_id'] >= 0).sum() > 500
        for k in full:
            assert part[k].shape[:2] == (H, W) and np.array_equal(part[k], full[k][:H, :W]), (H, W, k)


def test_host_route_does_not_depend_on_its_chunking(monkeypatch):
    verts, faces = soup(n=400, size=64, seed=2)
    col = vertex_colors(verts)
    whole = raster.rasterize_host(verts, faces, col, EYE_K, EYE_E, 64, 64)
    monkeypatch.setattr(raster, '_HOST_CHUNK', 1000)
    parts = raster.rasterize_host(verts, faces, col, EYE_K, EYE_E, 64, 64)
    assert (whole['tri_id'] >= 0).mean() > 0.9
    for k in whole:
        assert np.array_equal(whole[k], parts[k])


def test_abi_raster_argument_errors_do_not_need_a_gpu():
    from humannerf_amd import _lib
    lib = _lib.load()
    err = lambda: lib.hnrf_last_error().decode()
    p = 256                                                             # (a non-null, aligned stand-in: never read)
    call = lambda **kw: lib.hnrf_raster_mesh(*[kw.get(k, d) for k, d in (
        ('verts', p), ('V', 3), ('faces', p), ('F', 1), ('colors', p), ('K', p), ('R', p), ('T', p), ('bgcolor', p),
        ('H', 16), ('W', 16), ('z_near', 1e-3), ('flags', 0), ('rgb', p), ('alpha', p), ('depth', p), ('tri_id', p),
        ('workspace', p), ('workspace_bytes', 1 << 40), ('stream', None))])
    for k in ('verts', 'faces', 'K', 'R', 'T', 'workspace', 'bgcolor', 'colors'):
        assert call(**{k: None}) == -1 and 'null pointer' in err(), k
    assert call(H=0) == -2 and '0x16' in err()
    assert call(W=9000) == -2 and '9000' in err()
    assert call(V=2 ** 31) == -2 and call(F=2 ** 31) == -2 and call(V=-1) == -2
    assert call(z_near=0.0) == -2 and call(flags=3) == -2 and call(flags=8) == -2
    assert call(workspace_bytes=16) == -4
    assert call(workspace=p + 8) == -1 and 'aligned' in err()
    ws = lib.hnrf_raster_workspace_bytes
    assert ws(0, 0, 1, 1) > 0 and ws(3, 1, 16, 16) >= 3 * 12 + 16 * 16 * 8
    assert ws(1000, 100000, 64, 64) > ws(1000, 1000, 64, 64)
    assert ws(1000, 1000, 512, 512) >= ws(1000, 1000, 64, 64) + (512 * 512 - 64 * 64) * 8
    assert ws(2 ** 31, 1, 16, 16) == 0 and ws(3, 1, 0, 16) == 0 and ws(3, 1, 16, 9000) == 0
