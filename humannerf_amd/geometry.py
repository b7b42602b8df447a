"""Geometry maps of a rendered frame: depth, normal, shaded and non-rigid-offset panels (include/hnrf_geometry.h,
csrc/hnrf_geometry.hip).

By default (cfg.amd.maps_normals = 'screen') the normals are SCREEN-SPACE DIFFERENCES OF THE RENDERED SURFACE DISTANCE --
the per-ray depth the compositing kernel already returns, turned into a point per pixel and differenced along the image
axes.  They cost no network evaluation and are the same for the exact, culled and baked paths; they are not the gradient
of the density.  With cfg.amd.maps_normals = 'gradient' the 'normal' and 'shaded' panels are painted from
DENSITY-GRADIENT normals instead (include/hnrf_normals.h, csrc/hnrf_normals.hip): Network.ray_normals runs the training
kernels over the samples that carry weight and hnrf_ray_normals blends their unit normals per ray; the same gradient
gives meshes and glTF files their vertex normals (Network.vertex_normals).

  ray_normals_host, normal_panels_host,          the numpy twins of hnrf_normals.h, bit for bit
  field_normals_host

  ray_surface_host, pixel_rays_host, maps_host   the numpy twins: the second statement of every formula of the header,
                                                 bit for bit (fp32, every operation rounded on its own, the header's
                                                 orders of summation)
  frame_maps                                     the device entry the render loops call: three library calls in the
                                                 frame's launches, a workspace per (H, W, N), nothing synchronises

Maps are defined for cfg.perturb == 0 only (the render loops set it): with perturb > 0 the samples do not sit at z_at.
"""
import numpy as np

from .config import cfg

MAP_NAMES = ('depth', 'normal', 'shaded', 'offset')
SURFACES = ('expected', 'median')
OUTPUTS = ('normal', 'nvalid', 'normal8', 'depth8', 'shaded8', 'offset8')
OFFSET_MIN, OFFSET_MAX = -0.02, 0.02        # compare_lbs_delta.py:7 of the reference
AMBIENT, ALBEDO = 0.25, 0.8

_F = np.float32


# ------------------------------------------------------------------------------------------------------ numpy twins
def z_at_host(near, far, k, S):
    """csrc/hnrf_zat.h in numpy: the depth of sample k of S (k an integer array), fp32."""
    k = np.asarray(k, dtype=np.int64)
    with np.errstate(all='ignore'):
        step = _F(1) / _F(S - 1)
        t = np.where(k < S // 2, step * k.astype(_F), _F(1) - step * (S - 1 - k).astype(_F)).astype(_F)
        return (np.asarray(near, _F) * (_F(1) - t) + np.asarray(far, _F) * t).astype(_F)


def cumulative_host(weights):
    """The header's cumulative sum of (R, S) fp32 weights -> c (R, S): tiles of 64, Kogge-Stone within a tile, then
    c = fl(carry + v) and carry = c of the tile's last lane."""
    w = np.asarray(weights, dtype=_F)
    R, S = w.shape
    c = np.empty((R, S), _F)
    carry = np.zeros(R, _F)
    with np.errstate(all='ignore'):
        for s0 in range(0, S, 64):
            v = np.zeros((R, 64), _F)
            n = min(64, S - s0)
            v[:, :n] = w[:, s0:s0 + n]
            off = 1
            while off < 64:
                u = v.copy()
                v[:, off:] = u[:, off:] + u[:, :-off]
                off *= 2
            tile = carry[:, None] + v
            carry = tile[:, 63].copy()
            c[:, s0:s0 + n] = tile[:, :n]
    return c


def weighted_offsets_host(weights, offsets):
    """woff (R, 3) = sum_s w_s offset_s in the order of hnrf_surface_points: lane l of 64 adds the samples l, l + 64, ...
    ascending, then the butterfly over the lane distances 32 .. 1."""
    w = np.asarray(weights, dtype=_F)
    R, S = w.shape
    o = np.asarray(offsets, dtype=_F).reshape(R, S, 3)
    acc = np.zeros((R, 64, 3), _F)
    with np.errstate(all='ignore'):
        for s0 in range(0, S, 64):
            n = min(64, S - s0)
            acc[:, :n] = acc[:, :n] + w[:, s0:s0 + n, None] * o[:, s0:s0 + n]
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ off]
    return acc[:, 0].copy()


def ray_surface_host(near, far, alpha, depth, weights=None, offsets=None, alpha_min=0.5, want_median=False,
                     want_woff=False):
    """hnrf_ray_surface in numpy -> {'t_exp', 'valid' (uint8: bit 0 expected, bit 1 median), and when asked for 't_med',
    'k_med' (the median sample, -1 where there is none) and 'woff'}."""
    if (want_median or want_woff) and weights is None:
        raise ValueError('ray_surface_host: t_med and woff need weights (the lean form has t_exp only)')
    if want_woff and offsets is None:
        raise ValueError('ray_surface_host: woff needs offsets')
    a, d = np.asarray(alpha, _F).reshape(-1), np.asarray(depth, _F).reshape(-1)
    with np.errstate(all='ignore'):
        ok = np.isfinite(a) & np.isfinite(d) & (a >= _F(alpha_min))
        t_exp = np.where(ok, d / np.where(ok, a, _F(1)), _F(0)).astype(_F)
    res = {'t_exp': t_exp, 'valid': ok.astype(np.uint8)}
    if want_woff:
        res['woff'] = weighted_offsets_host(weights, offsets)
    if want_median:
        w = np.asarray(weights, _F)
        R, S = w.shape
        c = cumulative_host(w)
        with np.errstate(all='ignore'):
            total = c[:, S - 1]
            hit = c >= (_F(0.5) * total)[:, None]
            k = np.where(hit.any(axis=1), hit.argmax(axis=1), -1)
            k = np.where(ok & (total > 0), k, -1)
            z = z_at_host(np.asarray(near, _F).reshape(-1), np.asarray(far, _F).reshape(-1), np.maximum(k, 0), S)
            okm = (k >= 0) & np.isfinite(z)
        res['k_med'] = np.where(okm, k, -1).astype(np.int64)
        res['t_med'] = np.where(okm, z, _F(0)).astype(_F)
        res['valid'] = (res['valid'] | (okm.astype(np.uint8) << 1)).astype(np.uint8)
    return res


def pixel_rays_host(ray_index, H, W):
    """hnrf_pixel_rays in numpy -> (pix2ray (H * W,) int32 or None when the status is not 0, status)."""
    idx = np.asarray(ray_index, dtype=np.int64).reshape(-1)
    if ((idx < 0) | (idx >= H * W)).any():
        return None, 1
    p = np.full(H * W, -1, np.int32)
    np.maximum.at(p, idx, np.arange(idx.size, dtype=np.int32))
    return p, 0


def q8_host(v):
    """0 where !(v > 0), 255 where v >= 1, else trunc(255 v): render.to_8b_image with NaN -> 0."""
    v = np.asarray(v, dtype=_F)
    with np.errstate(all='ignore'):
        inside = (v > 0) & (v < 1)
        q = (_F(255) * np.where(inside, v, _F(0))).astype(np.int32)
        return np.where(v >= 1, 255, q).astype(np.uint8)


def offset_color_host(woff):
    """trunc(255 clip((woff + 0.02) / 0.04, 0, 1)) in fp32, NaN -> 0 (compare_lbs_delta.py:7-9, 47)."""
    with np.errstate(all='ignore'):
        v = (np.asarray(woff, _F) - _F(OFFSET_MIN)) / _F(OFFSET_MAX - OFFSET_MIN)
        vc = np.where(~(v > 0), _F(0), np.where(v > 1, _F(1), v)).astype(_F)
        return (vc * _F(255)).astype(np.int32).astype(np.uint8)


def _shift(a, dy, dx, fill):
    """a[y + dy, x + dx] with ``fill`` outside the image."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[yd, xd] = a[ys, xs]
    return out


def maps_host(rays_o, rays_d, surf, pix2ray, H, W, want=OUTPUTS, surface=0, alpha=None, edge=0.05, M=None, bgcolor=None,
              lohi=None, ambient=AMBIENT, albedo=ALBEDO, truth8=None):
    """hnrf_geometry_maps in numpy: ``surf`` = what ray_surface_host returned -> {name: array} for ``want``."""
    o, d = np.asarray(rays_o, _F).reshape(-1, 3), np.asarray(rays_d, _F).reshape(-1, 3)
    N = o.shape[0]
    p2r = np.asarray(pix2ray, np.int64).reshape(H, W)
    has_ray = (p2r >= 0) & (p2r < N)
    r = np.where(has_ray, p2r, 0)
    tarr = np.asarray(surf['t_med' if surface else 't_exp'], _F).reshape(-1) if N else np.zeros(1, _F)
    valid = np.asarray(surf['valid'], np.uint8).reshape(-1) if N else np.zeros(1, np.uint8)
    if N == 0:
        o, d = np.zeros((1, 3), _F), np.zeros((1, 3), _F)
    ok = has_ray & (((valid[r] >> surface) & 1) == 1)
    edge, ambient, albedo = _F(edge), _F(ambient), _F(albedo)
    bg = np.asarray(bgcolor, _F).reshape(3)
    bg8 = q8_host(bg)
    res = {}
    with np.errstate(all='ignore'):
        t = np.where(ok, tarr[r], _F(0)).astype(_F)
        P = (o[r] + d[r] * t[..., None]).astype(_F)

        def diff(dy, dx):
            tm, tp = _shift(t, -dy, -dx, _F(0)), _shift(t, dy, dx, _F(0))
            qm = _shift(ok, -dy, -dx, False) & (np.abs(t - tm) <= edge)
            qp = _shift(ok, dy, dx, False) & (np.abs(tp - t) <= edge)
            a = np.where(qp[..., None], _shift(P, dy, dx, _F(0)), P)
            b = np.where(qm[..., None], _shift(P, -dy, -dx, _F(0)), P)
            return (a - b).astype(_F), qm | qp

        A, hx = diff(0, 1)
        B, hy = diff(1, 0)
        cx = A[..., 1] * B[..., 2] - A[..., 2] * B[..., 1]
        cy = A[..., 2] * B[..., 0] - A[..., 0] * B[..., 2]
        cz = A[..., 0] * B[..., 1] - A[..., 1] * B[..., 0]
        ln = np.sqrt((cx * cx + cy * cy) + cz * cz).astype(_F)
        has = ok & hx & hy & (ln > 0) & np.isfinite(ln)
        safe = np.where(has, ln, _F(1))
        n = np.stack([cx / safe, cy / safe, cz / safe], -1).astype(_F)
        dr = d[r]
        nd = ((n[..., 0] * dr[..., 0] + n[..., 1] * dr[..., 1]) + n[..., 2] * dr[..., 2]).astype(_F)
        n = np.where((nd > 0)[..., None], -n, n)
        n = np.where(has[..., None], n, _F(0)).astype(_F)
        dl = np.sqrt((dr[..., 0] * dr[..., 0] + dr[..., 1] * dr[..., 1]) + dr[..., 2] * dr[..., 2]).astype(_F)
        if 'normal' in want:
            res['normal'] = n
        if 'nvalid' in want:
            res['nvalid'] = has.astype(np.uint8)
        if 'normal8' in want:
            m = np.asarray(M, _F).reshape(3, 3)
            mn = np.stack([(m[i, 0] * n[..., 0] + m[i, 1] * n[..., 1]) + m[i, 2] * n[..., 2] for i in range(3)], -1)
            res['normal8'] = np.where(has[..., None], q8_host(_F(0.5) + _F(0.5) * mn), bg8)
        if 'depth8' in want:
            lo, hi = np.asarray(lohi, _F).reshape(2)
            g = q8_host(_F(1) - (t - lo) / (hi - lo))
            res['depth8'] = np.where(ok[..., None], np.stack([g, g, g], -1), bg8)
        if 'shaded8' in want:
            a = np.asarray(alpha, _F).reshape(-1)[r] if N else np.zeros((H, W), _F)
            s = np.where(has, ambient + (_F(1) - ambient) * (np.abs(nd) / dl), ambient).astype(_F)
            ga, na = (s * albedo) * a, _F(1) - a
            col = np.stack([ga + na * bg[i] for i in range(3)], -1)
            res['shaded8'] = np.where(ok[..., None], q8_host(col), bg8)
        if 'offset8' in want:
            paint = has_ray & (np.asarray(truth8).reshape(H, W, 3).astype(np.int64).sum(-1) > 0) if truth8 is not None else ok
            woff = np.asarray(surf['woff'], _F).reshape(-1, 3) if N else np.zeros((1, 3), _F)
            res['offset8'] = np.where(paint[..., None], offset_color_host(woff[r]), np.uint8(0)).astype(np.uint8)
    return {k: np.ascontiguousarray(v) for k, v in res.items()}


# ------------------------------------------------------------------------- numpy twins of include/hnrf_normals.h
def _len3_host(v):
    """sqrt(fl(fl(fl(v0 v0) + fl(v1 v1)) + fl(v2 v2))) of (..., 3) fp32."""
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).astype(_F)


def ray_normals_host(weights, bmw, motion_Rs, idx, g, alpha, alpha_min=0.5):
    """hnrf_ray_normals in numpy: weights (R, S), bmw (R, S, B), motion_Rs (B, 3, 3), idx (n,) the kept samples as flat
    indices (distinct, in any order), g (n, 3) the skeleton-space density gradient at them, row k for idx[k], alpha (R,)
    -> (normal (R, 3) fp32, nvalid (R,) uint8)."""
    w = np.asarray(weights, dtype=_F)
    R, S = w.shape
    m = np.asarray(bmw, dtype=_F).reshape(R * S, -1)
    Rs = np.asarray(motion_Rs, dtype=_F).reshape(-1, 9)
    B = Rs.shape[0]
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    g = np.asarray(g, dtype=_F).reshape(-1, 3)[:idx.size]
    inside = (idx >= 0) & (idx < R * S)
    idx, g = idx[inside], g[inside]
    contrib = np.zeros((R * S, 3), _F)
    with np.errstate(all='ignore'):
        A = np.zeros((idx.size, 9), _F)
        mk = m[idx]
        for b in range(B):
            A = A + mk[:, b, None] * Rs[b][None, :]
        v = np.stack([-((A[:, j] * g[:, 0] + A[:, 3 + j] * g[:, 1]) + A[:, 6 + j] * g[:, 2]) for j in range(3)], -1).astype(_F)
        ln = _len3_host(v)
        good = (ln > 0) & np.isfinite(ln)
        u = v / np.where(good, ln, _F(1))[:, None]
        # (a sample that contributes nothing adds +0: acc starts at +0 and a sum never rounds to -0, so acc is unchanged)
        contrib[idx] = np.where(good[:, None], w.reshape(-1)[idx][:, None] * u, _F(0))
        contrib = contrib.reshape(R, S, 3)
        acc = np.zeros((R, 64, 3), _F)
        for s0 in range(0, S, 64):
            n = min(64, S - s0)
            acc[:, :n] = acc[:, :n] + contrib[:, s0:s0 + n]
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ off]
        N = acc[:, 0]
        L = _len3_host(N)
        a = np.asarray(alpha, _F).reshape(-1)
        ok = np.isfinite(a) & (a >= _F(alpha_min)) & (L > 0) & np.isfinite(L)
        normal = np.where(ok[:, None], N / np.where(ok, L, _F(1))[:, None], _F(0)).astype(_F)
    return np.ascontiguousarray(normal), ok.astype(np.uint8)


NORMAL_OUTPUTS = ('normal', 'nvalid', 'normal8', 'shaded8')


def normal_panels_host(rays_d, ray_normal, ray_nvalid, valid, pix2ray, H, W, want=NORMAL_OUTPUTS, surface=0, alpha=None,
                       M=None, bgcolor=None, ambient=AMBIENT, albedo=ALBEDO):
    """hnrf_normal_panels in numpy: per-ray normals (ray_normals_host), the valid bits of ray_surface_host and pix2ray
    -> {name: array} for ``want`` out of NORMAL_OUTPUTS."""
    d = np.asarray(rays_d, _F).reshape(-1, 3)
    N = d.shape[0]
    p2r = np.asarray(pix2ray, np.int64).reshape(H, W)
    has_ray = (p2r >= 0) & (p2r < N)
    r = np.where(has_ray, p2r, 0)
    if N == 0:
        d, rn, rv, valid = np.zeros((1, 3), _F), np.zeros((1, 3), _F), np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    else:
        rn, rv = np.asarray(ray_normal, _F).reshape(-1, 3), np.asarray(ray_nvalid, np.uint8).reshape(-1)
        valid = np.asarray(valid, np.uint8).reshape(-1)
    ok = has_ray & (((valid[r] >> surface) & 1) == 1)
    has = ok & (rv[r] != 0)
    ambient, albedo = _F(ambient), _F(albedo)
    bg = np.asarray(bgcolor, _F).reshape(3)
    bg8 = q8_host(bg)
    res = {}
    with np.errstate(all='ignore'):
        n = np.where(has[..., None], rn[r], _F(0)).astype(_F)
        if 'normal' in want:
            res['normal'] = n
        if 'nvalid' in want:
            res['nvalid'] = has.astype(np.uint8)
        if 'normal8' in want:
            m = np.asarray(M, _F).reshape(3, 3)
            mn = np.stack([(m[i, 0] * n[..., 0] + m[i, 1] * n[..., 1]) + m[i, 2] * n[..., 2] for i in range(3)], -1)
            res['normal8'] = np.where(has[..., None], q8_host(_F(0.5) + _F(0.5) * mn), bg8)
        if 'shaded8' in want:
            dr = d[r]
            nd = ((n[..., 0] * dr[..., 0] + n[..., 1] * dr[..., 1]) + n[..., 2] * dr[..., 2]).astype(_F)
            dl = np.sqrt((dr[..., 0] * dr[..., 0] + dr[..., 1] * dr[..., 1]) + dr[..., 2] * dr[..., 2]).astype(_F)
            a = np.asarray(alpha, _F).reshape(-1)[r] if N else np.zeros((H, W), _F)
            s = np.where(has, ambient + (_F(1) - ambient) * (np.abs(nd) / dl), ambient).astype(_F)
            ga, na = (s * albedo) * a, _F(1) - a
            col = np.stack([ga + na * bg[i] for i in range(3)], -1)
            res['shaded8'] = np.where(ok[..., None], q8_host(col), bg8)
    return {k: np.ascontiguousarray(v) for k, v in res.items()}


def trilinear_gradient_host(verts, vol, bbox_min, bbox_scale, n_bones=None):
    """fg (V,) and grad fg (V, 3) of hnrf_field_normals: the summed trilinear bone weights at canonical points and the
    analytic derivative of the trilinear weights, fp32, in the header's order."""
    from . import skin
    v = np.asarray(verts, _F).reshape(-1, 3)
    vol = np.asarray(vol, _F)
    bmin, bscale = np.asarray(bbox_min, _F).reshape(3), np.asarray(bbox_scale, _F).reshape(3)
    B, G = (vol.shape[0] if n_bones is None else int(n_bones)), vol.shape[-1]
    gm1 = _F(G - 1)
    off, cw = skin._trilinear_host(v, bmin, bscale, G)
    u, e = [], []
    with np.errstate(all='ignore'):
        for a in range(3):
            i = (((v[:, a] - bmin[a]) * bscale[a] - _F(1)) + _F(1)) * _F(0.5) * gm1
            f0 = np.floor(i)
            w1, w0 = i - f0, (f0 + _F(1)) - i
            x0 = np.fmin(np.fmax(f0, _F(-2)), gm1 + _F(1)).astype(np.int64)
            in0, in1 = (x0 >= 0) & (x0 < G), (x0 + 1 >= 0) & (x0 + 1 < G)
            u.append((np.where(in0, w0, _F(0)).astype(_F), np.where(in1, w1, _F(0)).astype(_F)))
            e.append((np.where(in0, _F(-1), _F(0)).astype(_F), np.where(in1, _F(1), _F(0)).astype(_F)))
        flat = vol[:B].reshape(B, -1)
        fg = np.zeros(len(v), _F)
        Gr = np.zeros((len(v), 3), _F)
        for b in range(B):
            w = np.zeros(len(v), _F)
            wd = np.zeros((len(v), 3), _F)
            for k in range(8):
                dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
                c = flat[b, off[:, k]]
                w = w + c * cw[:, k]
                wd[:, 0] = wd[:, 0] + c * (e[0][dx] * u[1][dy] * u[2][dz])
                wd[:, 1] = wd[:, 1] + c * (u[0][dx] * e[1][dy] * u[2][dz])
                wd[:, 2] = wd[:, 2] + c * (u[0][dx] * u[1][dy] * e[2][dz])
            fg = fg + w
            Gr = Gr + wd
        grad = (Gr * ((bscale * _F(0.5)) * gm1)[None, :]).astype(_F)
    return fg, grad


def field_normals_host(verts, g, sigma, vol, bbox_min, bbox_scale, n_bones=None):
    """hnrf_field_normals in numpy: the unit normal -grad D / |grad D| of D = relu(sigma) fg at canonical points
    (V, 3), from grad sigma ``g`` (V, 3) and ``sigma`` (V,) there; 0 where the length is 0 or not finite."""
    fg, gfg = trilinear_gradient_host(verts, vol, bbox_min, bbox_scale, n_bones)
    g, sg = np.asarray(g, _F).reshape(-1, 3), np.asarray(sigma, _F).reshape(-1)
    with np.errstate(all='ignore'):
        pos = sg > 0
        sr = np.where(pos, sg, _F(0)).astype(_F)
        gs = np.where(pos[:, None], g, _F(0)).astype(_F)
        D = (fg[:, None] * gs + sr[:, None] * gfg).astype(_F)
        ln = _len3_host(D)
        ok = (ln > 0) & np.isfinite(ln)
        n = np.where(ok[:, None], -(D / np.where(ok, ln, _F(1))[:, None]), _F(0)).astype(_F)
    return np.ascontiguousarray(n)


# -------------------------------------------------------------------------------------------------- the device entry
def check_maps(maps, surface='expected', diagnostics=True):
    """The panel names and the surface a caller asks for; ValueError names what is wrong."""
    maps = list(maps)
    bad = [m for m in maps if m not in MAP_NAMES]
    if bad or len(set(maps)) != len(maps):
        raise ValueError('maps must be distinct names out of %r, got %r' % (MAP_NAMES, maps))
    if surface not in SURFACES:
        raise ValueError('surface must be one of %r, got %r' % (SURFACES, surface))
    if not diagnostics and ('offset' in maps or surface == 'median'):
        raise ValueError("the 'offset' map (cfg.amd.maps) and the 'median' surface (cfg.amd.maps_surface) need the per-sample "
                         "weights and offsets: set cfg.amd.diagnostics = True (the lean form has neither)")
    return maps


_WORKSPACES = {}


def _workspace(H, W, N, device):
    import torch
    key = (H, W, N, str(device))
    ws = _WORKSPACES.get(key)
    if ws is None:
        if len(_WORKSPACES) >= 8:                        # a loop renders one size; a few are kept
            _WORKSPACES.pop(next(iter(_WORKSPACES)))
        u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=device)
        ws = {'t_exp': torch.empty(N, device=device), 't_med': torch.empty(N, device=device),
              'woff': torch.empty(N, 3, device=device), 'valid': u8(N),
              'pix2ray': torch.empty(H * W, dtype=torch.int32, device=device),
              'status': torch.zeros(1, dtype=torch.int32, device=device), 'lohi': torch.empty(2, device=device),
              'c255': torch.full((1,), 255., device=device), 'eye': torch.eye(3, device=device),
              'normal': torch.empty(H, W, 3, device=device), 'nvalid': u8(H, W)}
        _WORKSPACES[key] = ws
    return ws


def frame_maps(data, out, H, W, ray_index, maps=MAP_NAMES, surface='expected', alpha_min=0.5, edge=0.05, M=None,
               truth8=None, ray_normals=None):
    """The panels of one rendered frame on the device.  ``data``: the frame's inputs as the network got them (``rays``
    (2, N, 3), ``near``, ``far``, ``bgcolor`` in 0..255); ``out``: what the network returned (``alpha``, ``depth`` and,
    with cfg.amd.diagnostics, ``weights_on_rays`` and ``offsets``); ``ray_index`` (N,) int64 the flat pixel of every ray;
    ``M`` (3, 3) the world-to-camera rotation for the normal panel (None = identity); ``truth8`` (H, W, 3) uint8 or
    None (where the offset panel is painted).  Returns {name: uint8 tensor (H, W, 3)} for ``maps`` plus ``normal_world``
    (H, W, 3) fp32 (the unit normals in world space; 'normal' is the 8-bit panel), ``nvalid`` (H, W) uint8, ``t`` (N,)
    and ``status`` (1,) int32 (not read back: 0 = fine, 1 = a ray index outside the image, and then nothing was
    written).  The panels are fresh tensors; normal_world, nvalid and t live in
    a workspace per (H, W, N) that the next frame of that size overwrites.  Nothing here synchronises.
    ``ray_normals``: (normal (N, 3), nvalid (N,) uint8) of Network.ray_normals -- the 'normal' and 'shaded' panels,
    normal_world and nvalid then come from hnrf_normal_panels (density-gradient normals, not flipped towards the
    camera); 'depth' and 'offset' stay as they are."""
    import torch
    from . import ops
    if float(cfg.perturb) > 0.:
        raise ValueError('geometry maps are defined for cfg.perturb == 0 only (got %r): with stratified sampling the '
                         'samples do not sit at z_at' % (cfg.perturb,))
    diag = 'weights_on_rays' in out and 'offsets' in out
    maps = check_maps(maps, surface, diag)
    H, W = int(H), int(W)
    rays = data['rays']
    rays_o, rays_d = rays[0].reshape(-1, 3).contiguous(), rays[1].reshape(-1, 3).contiguous()
    N, dev = rays_o.shape[0], rays_o.device
    if dev.type != 'cuda':
        raise ValueError('geometry maps need a GPU (got device %s); on the host use geometry.maps_host' % dev)
    ws = _workspace(H, W, N, dev)
    near, far = data['near'].reshape(-1).contiguous(), data['far'].reshape(-1).contiguous()
    median, want_woff = surface == 'median', 'offset' in maps
    S = int(out['weights_on_rays'].shape[-1]) if diag else 1
    surf = ops.ray_surface(near, far, out['alpha'].reshape(-1), out['depth'].reshape(-1),
                           out['weights_on_rays'].reshape(N, S) if (median or want_woff) else None,
                           out['offsets'].reshape(N, S, 3) if want_woff else None, alpha_min=alpha_min,
                           want_median=median, want_woff=want_woff, out=ws)
    ops.pixel_rays(ray_index, H, W, pix2ray=ws['pix2ray'], status=ws['status'])
    # (by a tensor: torch divides by a Python scalar as a product with its reciprocal, which is not the twin's division)
    bg = (data['bgcolor'].reshape(3).to(torch.float32) / ws['c255']).contiguous()
    if 'depth' in maps:
        if N:
            torch.stack([near.min(), far.max()], out=ws['lohi'])
        else:
            ws['lohi'].zero_()
    Mt = ws['eye'] if M is None else torch.as_tensor(M, dtype=torch.float32).to(dev).contiguous()
    names = {'depth': 'depth8', 'normal': 'normal8', 'shaded': 'shaded8', 'offset': 'offset8'}
    if ray_normals is not None:
        # normal, nvalid and the two panels made of normals from the per-ray normals; depth and offset as ever
        rn, rv = ray_normals
        other = [names[m] for m in maps if m in ('depth', 'offset')]
        res = ops.geometry_maps(rays_o, rays_d, surf, ws['pix2ray'], H, W, other, surface=int(median),
                                alpha=out['alpha'].reshape(-1), edge=edge, M=Mt, bgcolor=bg, lohi=ws['lohi'],
                                truth8=truth8 if want_woff else None, status=ws['status']) if other else {}
        res.update(ops.normal_panels(rays_d, rn.reshape(-1, 3).contiguous(), rv.reshape(-1).contiguous(), surf['valid'],
                                     ws['pix2ray'], H, W,
                                     ['normal', 'nvalid'] + [names[m] for m in maps if m in ('normal', 'shaded')],
                                     surface=int(median), alpha=out['alpha'].reshape(-1).contiguous(), M=Mt, bgcolor=bg,
                                     ambient=AMBIENT, albedo=ALBEDO, status=ws['status'],
                                     out={'normal': ws['normal'], 'nvalid': ws['nvalid']}))
        ret = {m: res[names[m]] for m in maps}
        ret.update(normal_world=res['normal'], nvalid=res['nvalid'], t=surf['t_med' if median else 't_exp'],
                   status=ws['status'])
        return ret
    res = ops.geometry_maps(rays_o, rays_d, surf, ws['pix2ray'], H, W, ['normal', 'nvalid'] + [names[m] for m in maps],
                            surface=int(median), alpha=out['alpha'].reshape(-1), edge=edge, M=Mt, bgcolor=bg,
                            lohi=ws['lohi'], truth8=truth8 if want_woff else None, status=ws['status'],
                            out={'normal': ws['normal'], 'nvalid': ws['nvalid']})
    ret = {m: res[names[m]] for m in maps}
    ret.update(normal_world=res['normal'], nvalid=res['nvalid'], t=surf['t_med' if median else 't_exp'], status=ws['status'])
    return ret
