"""Scenes shared by tests/test_geometry_refs.py and tests/test_gpu_geometry.py: a pinhole camera at (0, 0, 3) looking
down -z with focal length 100 px, and analytic surfaces whose ray distances are computed in fp64.  Not a test."""
import numpy as np

CAM = np.array([0.0, 0.0, 3.0])
FOCAL = 100.0
PLANES = [(0.0, 0.0, 1.0), (0.3, 0.2, 1.0), (1.0, 0.0, 1.0), (0.5, -0.8, 0.6)]
S_LIST = (1, 2, 63, 64, 65, 128, 300)


def camera(H, W):
    """(o (H W, 3), d (H W, 3)) in fp64, rays in pixel order, d = ((x - W / 2) / f, (y - H / 2) / f, -1): not normalised,
    the principal point at (W / 2, H / 2)."""
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.stack([(xs - W / 2.0) / FOCAL, (ys - H / 2.0) / FOCAL, -np.ones((H, W))], -1).reshape(-1, 3)
    return np.tile(CAM, (H * W, 1)), d


def full_frame(H, W, t64, hit=None):
    """The twin's inputs for a frame with one ray per pixel: t_exp = fl32(t64) where ``hit`` (default everywhere)."""
    o, d = camera(H, W)
    hit = np.ones(H * W, bool) if hit is None else hit.reshape(-1)
    t = np.where(hit, t64.reshape(-1), 0.0).astype(np.float32)
    surf = {'t_exp': t, 'valid': hit.astype(np.uint8)}
    return o.astype(np.float32), d.astype(np.float32), surf, np.arange(H * W, dtype=np.int32)


def plane_t(n, c, H, W):
    """fp64 distance along every ray to the plane n.x = c."""
    o, d = camera(H, W)
    n = np.asarray(n, np.float64)
    return (c - o @ n) / (d @ n)


def sphere_t(r, H, W):
    """(t64, hit): the near intersection with the sphere of radius r at the origin."""
    o, d = camera(H, W)
    a, b, c = (d * d).sum(1), 2 * (o * d).sum(1), (o * o).sum(1) - r * r
    disc = b * b - 4 * a * c
    hit = disc > 0
    return np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), 0.0), hit


def step_t(H, W, col, gap=0.2):
    """Two fronto-parallel planes: z = 0 left of column ``col``, z = -gap from it on."""
    x = np.tile(np.arange(W), H)
    return np.where(x < col, 3.0, 3.0 + gap)


def angle_deg(a, b):
    """atan2(|a x b|, a.b) in fp64, degrees (arccos loses half the digits near 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1)))


def surface_inputs(R, S, seed):
    """Random inputs of hnrf_ray_surface with every special row the issue names: (near, far, alpha, depth, weights,
    offsets) in fp32.  Rows 0..7 (where R allows): all-zero weights, one-hot at 0, one-hot at S - 1, all ones, a NaN
    weight, near == far, alpha just below 0.5, alpha just above it."""
    rs = np.random.RandomState(seed)
    w = (rs.uniform(0, 1, (R, S)) ** 3 * (rs.uniform(0, 1, (R, S)) < 0.6)).astype(np.float32)
    off = rs.normal(0, 0.02, (R, S, 3)).astype(np.float32)
    near = rs.uniform(0.5, 2.0, R).astype(np.float32)
    far = (near + rs.uniform(0.5, 2.0, R)).astype(np.float32)
    alpha = rs.uniform(0.0, 1.0, R).astype(np.float32)
    depth = (alpha * rs.uniform(0.5, 4.0, R)).astype(np.float32)
    special = [lambda r: w.__setitem__(r, 0.0),
               lambda r: (w.__setitem__(r, 0.0), w.__setitem__((r, 0), 1.0)),
               lambda r: (w.__setitem__(r, 0.0), w.__setitem__((r, S - 1), 1.0)),
               lambda r: w.__setitem__(r, 1.0),
               lambda r: w.__setitem__((r, S // 2), np.nan),
               lambda r: far.__setitem__(r, near[r]),
               lambda r: alpha.__setitem__(r, np.nextafter(np.float32(0.5), np.float32(0))),
               lambda r: alpha.__setitem__(r, np.nextafter(np.float32(0.5), np.float32(1)))]
    for r, f in enumerate(special[:R]):
        f(r)
        if r < 6:
            alpha[r] = 0.9
    if R > 9:
        alpha[8], depth[9] = np.nan, np.inf
    return near, far, alpha, depth, w, off
