"""Inputs and fp64 restatements shared by tests/test_normals_refs.py (CPU) and tests/test_gpu_normals.py (GPU): the
density-gradient normals of include/hnrf_normals.h.  The restatements are written on their own, in float64, without the
twins' orders of summation; the twins are held to them, the kernels to the twins."""
import numpy as np

S_LIST = [2, 64, 65, 130]               # the lane-stride edges: below a wave, one full wave, one over, two strides and a rest
WEIGHT_MIN = 1e-2
EPS_CANONICAL = 2e-5                    # what tests/test_gpu_train_kernels.py holds d_x to, of the largest element


def rotations(B, rs):
    q, _ = np.linalg.qr(rs.standard_normal((B, 3, 3)))
    return (q + 0.01 * rs.standard_normal((B, 3, 3))).astype(np.float32)       # (not exactly orthonormal, as the basis is)


def ray_case(R, S, B=24, seed=0, kept='mixed'):
    """weights (R, S), bmw (R, S, B), motion_Rs (B, 3, 3), idx (n,) int32 (w >= WEIGHT_MIN, ascending; a NaN is not
    kept, as hnrf_compact_samples), g (n, 3), alpha (R,).  ``kept``: 'none' | 'one' | 'all' per ray, or 'mixed': the rows
    cycle through none, one, all and random; zero gradients and non-finite / small alphas are strewn in."""
    rs = np.random.RandomState(seed)
    w = rs.uniform(0.02, 1.0, (R, S)).astype(np.float32)
    low = rs.uniform(0.0, 0.009, (R, S)).astype(np.float32)
    for r in range(R):
        kind = kept if kept != 'mixed' else ('none', 'one', 'all', 'random')[r % 4]
        if kind == 'none':
            w[r] = low[r]
        elif kind == 'one':
            k = rs.randint(S)
            keep = w[r, k]
            w[r] = low[r]
            w[r, k] = keep
        elif kind == 'random':
            drop = rs.uniform(size=S) < 0.5
            w[r, drop] = low[r, drop]
    if kept == 'mixed' and R * S > 4:
        w.reshape(-1)[rs.randint(R * S)] = np.nan
    bmw = rs.uniform(0.0, 1.0, (R, S, B)).astype(np.float32) ** 4
    Rs = rotations(B, rs)
    idx = np.nonzero(w.reshape(-1) >= np.float32(WEIGHT_MIN))[0].astype(np.int32)
    g = (rs.standard_normal((idx.size, 3)) * 100).astype(np.float32)
    if idx.size:
        g[rs.uniform(size=idx.size) < 0.1] = 0
    alpha = rs.uniform(0.3, 1.0, R).astype(np.float32)
    if kept == 'mixed' and R > 2:
        alpha[rs.randint(R)] = np.nan
    return w, bmw, Rs, idx, g, alpha


def ray_normals_fp64(w, bmw, Rs, idx, g, alpha, alpha_min=0.5):
    """The definition in float64: N = sum over the kept samples of w u, u = -A^T g / |A^T g|, A = sum_b bmw_b R_b."""
    R, S = w.shape
    w64, m64 = w.astype(np.float64).reshape(-1), bmw.astype(np.float64).reshape(R * S, -1)
    N = np.zeros((R, 3))
    for k, p in enumerate(idx):
        A = np.einsum('b,bij->ij', m64[p], Rs.astype(np.float64))
        v = -(A.T @ g[k].astype(np.float64))
        ln = np.linalg.norm(v)
        if ln > 0 and np.isfinite(ln):
            N[p // S] += w64[p] * v / ln
    L = np.linalg.norm(N, axis=1)
    with np.errstate(all='ignore'):
        ok = np.isfinite(alpha) & (alpha >= np.float32(alpha_min)) & (L > 0) & np.isfinite(L)
        return np.where(ok[:, None], N / np.where(ok, L, 1.0)[:, None], 0.0), ok


def panel_case(H, W, seed=0):
    """N rays on an H x W image: two rays share a pixel (when there are two), some pixels have no ray; per-ray normals,
    nvalid, valid bits, alpha, directions, a rotation M and a background."""
    rs = np.random.RandomState(seed)
    HW = H * W
    N = max(1, (HW * 3) // 4)
    ray_index = rs.permutation(HW)[:N].astype(np.int64)
    if N >= 2:
        ray_index[-1] = ray_index[0]                                       # the highest n wins
    n = rs.standard_normal((N, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    nvalid = (rs.uniform(size=N) < 0.7).astype(np.uint8)
    n[nvalid == 0] = 0
    valid = rs.randint(0, 4, N).astype(np.uint8)
    if N == 1:
        nvalid[:], valid[:] = 1, 3
    alpha = rs.uniform(0.0, 1.0, N).astype(np.float32)
    d = (rs.standard_normal((N, 3)) + np.array([0, 0, 3.0])).astype(np.float32)
    M = rotations(1, rs)[0]
    bg = rs.uniform(0, 1, 3).astype(np.float32)
    return dict(ray_index=ray_index, normal=n, nvalid=nvalid, valid=valid, alpha=alpha, rays_d=d, M=M, bgcolor=bg, N=N)


def panels_fp64(c, p2r, H, W, surface=0, ambient=0.25, albedo=0.8):
    """normal8 / shaded8 as real numbers in [0, 255] before truncation (float64), has (H, W), ok (H, W)."""
    p2r = np.asarray(p2r).reshape(H, W)
    has_ray = p2r >= 0
    r = np.where(has_ray, p2r, 0)
    ok = has_ray & (((c['valid'][r] >> surface) & 1) == 1)
    has = ok & (c['nvalid'][r] != 0)
    n = np.where(has[..., None], c['normal'][r].astype(np.float64), 0.0)
    bg = c['bgcolor'].astype(np.float64)
    n8 = np.where(has[..., None], 255.0 * np.clip(0.5 + 0.5 * n @ c['M'].astype(np.float64).T, 0, 1), 255.0 * bg)
    d = c['rays_d'][r].astype(np.float64)
    s = np.where(has, ambient + (1 - ambient) * np.abs((n * d).sum(-1)) / np.linalg.norm(d, axis=-1), ambient)
    a = c['alpha'][r].astype(np.float64)
    col = (s * albedo * a)[..., None] + (1 - a)[..., None] * bg
    s8 = np.where(ok[..., None], 255.0 * np.clip(col, 0, 1), 255.0 * bg)
    return n8, s8, has, ok


def field_case(V, B=24, G=8, seed=0):
    """verts (V, 3) inside and a little outside the box, g (V, 3), sigma (V,) of both signs, vol (B + 1, G, G, G)."""
    rs = np.random.RandomState(seed)
    bmin = np.array([-1.0, -1.2, -0.8], np.float32)
    bmax = np.array([1.1, 1.0, 0.9], np.float32)
    scale = (np.float32(2.0) / (bmax - bmin)).astype(np.float32)
    verts = (bmin + (bmax - bmin) * rs.uniform(-0.1, 1.1, (V, 3))).astype(np.float32)
    vol = rs.uniform(0.0, 1.0, (B + 1, G, G, G)).astype(np.float32)
    vol /= vol.sum(0, keepdims=True)
    g = (rs.standard_normal((V, 3)) * 100).astype(np.float32)
    sigma = (rs.standard_normal(V) * 30).astype(np.float32)
    if V > 3:
        g[1] = 0
        sigma[2] = 0
    return verts, g, sigma, vol, bmin, scale


def fg_fp64(x, vol, bmin, scale, B):
    """The gate in float64, written on its own: align_corners trilinear interpolation with zero padding of the B bone
    channels, summed."""
    G = vol.shape[-1]
    i = (np.asarray(x, np.float64) - bmin.astype(np.float64)) * scale.astype(np.float64) * 0.5 * (G - 1)
    f = np.floor(i).astype(np.int64)
    t = i - f
    tot = 0.0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ix, iy, iz = f[0] + dx, f[1] + dy, f[2] + dz
                if not (0 <= ix < G and 0 <= iy < G and 0 <= iz < G):
                    continue
                wgt = (t[0] if dx else 1 - t[0]) * (t[1] if dy else 1 - t[1]) * (t[2] if dz else 1 - t[2])
                tot += wgt * vol[:B, iz, iy, ix].astype(np.float64).sum()
    return tot


def field_normals_fp64(verts, g, sigma, vol, bmin, scale, B, h=1e-6):
    """-grad D / |grad D| of D = relu(sigma) fg in float64, grad fg by central differences (valid away from cell
    faces)."""
    out = np.zeros((len(verts), 3))
    for v, x in enumerate(verts.astype(np.float64)):
        fg = fg_fp64(x, vol, bmin, scale, B)
        gfg = np.array([(fg_fp64(x + h * e, vol, bmin, scale, B) - fg_fp64(x - h * e, vol, bmin, scale, B)) / (2 * h)
                        for e in np.eye(3)])
        pos = sigma[v] > 0
        D = fg * (g[v].astype(np.float64) if pos else 0.0) + max(float(sigma[v]), 0.0) * gfg
        ln = np.linalg.norm(D)
        if ln > 0:
            out[v] = -D / ln
    return out


def away_from_faces(verts, bmin, scale, G, margin=1e-3):
    """True where no lattice coordinate of the vertex lies within ``margin`` of an integer (the derivative jumps there)."""
    i = (verts.astype(np.float64) - bmin) * scale * 0.5 * (G - 1)
    return (np.abs(i - np.rint(i)) > margin).all(axis=1)


def angle(a, b):
    """The angle in radians between rows of vectors (float64), as atan2(|a x b|, a.b): the arc cosine of a dot product
    near 1 resolves nothing below the square root of its rounding (4e-4 rad for fp32 unit vectors)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))
