"""Deterministic rasteriser for vertex-coloured triangle meshes: the preview of the posed avatar mesh.

``rasterize`` runs on the device (hnrf_raster_mesh, include/hnrf.h: a 64-bit visibility buffer folded with atomic
maxima, then one resolve pass); ``rasterize_host`` restates it in numpy, bit for bit (the host/device idiom of ``mesh``
and ``imageproc``).  Both follow these conventions; every float operation is rounded on its own (no fused
multiply-add, correctly rounded division and square root) and sums are associated left to right as written.

- Camera: a frame dict's ``K`` (3, 3) and ``E`` (4, 4), R = E[:3, :3], T = E[:3, 3].  In float32:
  ``xc_i = ((R_i0 x + R_i1 y) + R_i2 z) + T_i``, ``p_i = (K_i0 xc_0 + K_i1 xc_1) + K_i2 xc_2``, ``u = p_0 / p_2``,
  ``v = p_1 / p_2``, depth ``z = xc_2``, inverse depth ``w = 1 / z``.
- Sample points: pixel (i, j) (column, row) is sampled at screen position (i, j) exactly, where
  ``scene.get_rays_from_KRT`` shoots its ray; a mesh picture and a volume picture of one frame line up.
- Snapping: ``X = rint(256 u)``, ``Y = rint(256 v)`` (round half to even), integers; coverage is exact 64-bit integer
  arithmetic on them.  With ``a = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0)`` and ``s = sign(a)``, the edge values at
  the sample S = (256 i, 256 j) are ``E0 = s cross(P2 - P1, S - P1)``, ``E1 = s cross(P0 - P2, S - P2)``,
  ``E2 = s cross(P1 - P0, S - P0)`` (``cross(d, q) = d_x q_y - d_y q_x``), so that E0 + E1 + E2 = |a|.
- Dropped whole: a triangle with a vertex index outside [0, V), with a vertex that fails
  ``z >= z_near and |u| <= 16384 and |v| <= 16384 and w > 0`` (any comparison with a NaN fails; no clipping is built:
  the render loops' cameras are outside the body), or with a = 0.
- Fill rule: top-left on the snapped positions in the triangle's own positive orientation, so that it does not
  depend on the winding: the sample is inside iff for every edge E_k > 0, or E_k = 0 and the oriented edge vector
  d = s (edge k's vector above) has ``d_y < 0`` (a left edge) or ``d_y = 0 and d_x > 0`` (a top edge) -- the same as
  sampling at (i + eps, j + eps^2).  Two triangles that share an edge never both own a sample on it, never both miss it.
- Culling: ``cull`` = 'none' | 'back' | 'front'.  A triangle is front-facing when its winding normal
  (v1 - v0) x (v2 - v0) -- which ``mesh`` points outward -- faces the camera: ``(a < 0) != (det(K R) < 0)``, the
  determinant in float32, ``M = K R`` with ``M_ij = (K_i0 R_0j + K_i1 R_1j) + K_i2 R_2j`` and
  ``det = (M00 (M11 M22 - M12 M21) - M01 (M10 M22 - M12 M20)) + M02 (M10 M21 - M11 M20)``.
- Depth: in float64, ``b_k = E_k / |a|`` and ``w = (w0 + b1 (w1 - w0)) + b2 (w2 - w0)``, rounded to float32; a sample
  whose w is not > 0 is skipped.  The visible triangle of a pixel has the largest w, among equal w the lowest index
  (the key ``bits(w) << 32 | 0xFFFFFFFF - index`` is folded with a maximum, so the order of processing does not matter).
- Outputs for an H x W image: ``tri_id`` int32 (-1 = background), ``depth`` float32 ``1 / w`` (0 on background),
  ``alpha`` float32 1 / 0, ``rgb`` float32 (H, W, 3): ``bgcolor`` (0..1) on background; with ``shade='color'`` the
  perspective-correct mix of the vertex colours, in float64 ``q_k = b_k w_k``, ``((q0 c0 + q1 c1) + q2 c2) /
  ((q0 + q1) + q2)``, rounded to float32; with ``shade='normal'`` ``0.5 + 0.5 n_i``, ``n = R m`` (summed like xc
  without T), ``m = c / sqrt((c_x c_x + c_y c_y) + c_z c_z)``, ``c = (v1 - v0) x (v2 - v0) = (a_y b_z - a_z b_y,
  a_z b_x - a_x b_z, a_x b_y - a_y b_x)`` of the float32 world positions, all in float32 (m = 0 when the length is 0
  or not finite).  The winding normal is not flipped toward the viewer.  No lighting, no anti-aliasing.
"""
import numpy as np

GUARD_BAND = 16384.0
CULL = {'none': 0, 'back': 1, 'front': 2}
SHADE = {'color': 0, 'normal': 4}                # hnrf.h: HNRF_RASTER_SHADE_NORMAL
_HOST_CHUNK = 1 << 22                            # bbox samples per vectorised pass of the host route


def _np(a, dtype):
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=dtype))


def _check(verts, faces, colors, K, E, H, W, cull, shade, z_near):
    if cull not in CULL or shade not in SHADE:
        raise ValueError('cull must be one of %s and shade one of %s' % (sorted(CULL), sorted(SHADE)))
    if not (1 <= int(H) <= 8192 and 1 <= int(W) <= 8192):
        raise ValueError('image size %sx%s out of range [1, 8192]' % (H, W))
    if not (float(z_near) > 0.0 and np.isfinite(float(z_near))):
        raise ValueError('z_near must be positive and finite')
    if tuple(verts.shape[1:]) != (3,) or tuple(faces.shape[1:]) != (3,) or tuple(K.shape) != (3, 3) or \
            tuple(E.shape) != (4, 4):
        raise ValueError('verts (V, 3), faces (F, 3), K (3, 3), E (4, 4) expected')
    if shade == 'color' and (colors is None or tuple(colors.shape) != tuple(verts.shape)):
        raise ValueError("shade='color' needs colors (V, 3)")


def camera_flips(K, R):
    """det(K R) < 0 in float32 with the operation order of the module docstring."""
    K, R = np.asarray(K, np.float32), np.asarray(R, np.float32)
    M = [[(K[i, 0] * R[0, j] + K[i, 1] * R[1, j]) + K[i, 2] * R[2, j] for j in range(3)] for i in range(3)]
    det = (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])) + \
        M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0])
    return bool(det < 0)


def project_host(verts, K, E, z_near=1e-3):
    """Setup pass: snapped positions X, Y (int64), inverse depth w (float32), validity (bool), each (V,)."""
    v = _np(verts, np.float32).reshape(-1, 3)
    K, E = _np(K, np.float32), _np(E, np.float32)
    R, T = E[:3, :3], E[:3, 3]
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all='ignore'):
        xc = [((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + T[i] for i in range(3)]
        p = [(K[i, 0] * xc[0] + K[i, 1] * xc[1]) + K[i, 2] * xc[2] for i in range(3)]
        u, vv = p[0] / p[2], p[1] / p[2]
        w = np.float32(1.0) / xc[2]
        ok = (xc[2] >= np.float32(z_near)) & (np.abs(u) <= np.float32(GUARD_BAND)) & \
            (np.abs(vv) <= np.float32(GUARD_BAND)) & (w > 0)
        X = np.where(ok, np.rint(np.float32(256.0) * np.where(ok, u, 0)), 0).astype(np.int64)
        Y = np.where(ok, np.rint(np.float32(256.0) * np.where(ok, vv, 0)), 0).astype(np.int64)
    return X, Y, np.where(ok, w, np.float32(0)).astype(np.float32), ok


def _edges(P, s, sx, sy):
    """Oriented edge values E0, E1, E2 (int64) of triangles P = ((X0, Y0), (X1, Y1), (X2, Y2)) at samples (sx, sy)."""
    (X0, Y0), (X1, Y1), (X2, Y2) = P
    e0 = s * ((X2 - X1) * (sy - Y1) - (Y2 - Y1) * (sx - X1))
    e1 = s * ((X0 - X2) * (sy - Y2) - (Y0 - Y2) * (sx - X2))
    e2 = s * ((X1 - X0) * (sy - Y0) - (Y1 - Y0) * (sx - X0))
    return e0, e1, e2


def _inv_depth(e1, e2, A, w0, w1, w2):
    b1, b2 = e1.astype(np.float64) / A.astype(np.float64), e2.astype(np.float64) / A.astype(np.float64)
    w0, w1, w2 = w0.astype(np.float64), w1.astype(np.float64), w2.astype(np.float64)
    return ((w0 + b1 * (w1 - w0)) + b2 * (w2 - w0)).astype(np.float32)


def visibility_host(X, Y, w, ok, faces, H, W, cull='none', flip=False):
    """The visibility buffer (H, W) uint64: per pixel the largest key of the samples owned there, 0 = background."""
    f = _np(faces, np.int64).reshape(-1, 3)
    V = X.shape[0]
    keys = np.zeros(H * W, dtype=np.uint64)
    inr = np.all((f >= 0) & (f < V), axis=1)
    tri = np.nonzero(inr)[0]
    f = f[tri]
    good = ok[f].all(axis=1)
    tri, f = tri[good], f[good]
    P = [(X[f[:, k]], Y[f[:, k]]) for k in range(3)]
    area = (P[1][0] - P[0][0]) * (P[2][1] - P[0][1]) - (P[1][1] - P[0][1]) * (P[2][0] - P[0][0])
    keep = area != 0
    front = (area < 0) != bool(flip)
    if cull == 'back':
        keep &= front
    elif cull == 'front':
        keep &= ~front
    i0 = np.maximum((np.minimum(np.minimum(P[0][0], P[1][0]), P[2][0]) + 255) >> 8, 0)
    i1 = np.minimum(np.maximum(np.maximum(P[0][0], P[1][0]), P[2][0]) >> 8, W - 1)
    j0 = np.maximum((np.minimum(np.minimum(P[0][1], P[1][1]), P[2][1]) + 255) >> 8, 0)
    j1 = np.minimum(np.maximum(np.maximum(P[0][1], P[1][1]), P[2][1]) >> 8, H - 1)
    keep &= (i1 >= i0) & (j1 >= j0)
    sgn = np.sign(area)
    thr = []                                     # per edge: 0 where the oriented edge is a top or left edge, else 1
    for a_, b_ in ((1, 2), (2, 0), (0, 1)):
        dx, dy = sgn * (P[b_][0] - P[a_][0]), sgn * (P[b_][1] - P[a_][1])
        thr.append(np.where((dy < 0) | ((dy == 0) & (dx > 0)), 0, 1).astype(np.int64))
    sel = np.nonzero(keep)[0]
    nx, ny = (i1 - i0 + 1)[sel], (j1 - j0 + 1)[sel]
    n = nx * ny
    start = 0
    while start < len(sel):
        stop = start + max(1, int(np.searchsorted(np.cumsum(n[start:]), _HOST_CHUNK, side='right')))
        g, cnt, gx = sel[start:stop], n[start:stop], nx[start:stop]
        start = stop
        t = np.repeat(np.arange(len(g)), cnt)                               # sample -> triangle of this pass
        k = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        gt = g[t]
        pi, pj = i0[gt] + k % gx[t], j0[gt] + k // gx[t]
        s = sgn[gt]
        Pt = [(P[c][0][gt], P[c][1][gt]) for c in range(3)]
        e = _edges(Pt, s, pi * 256, pj * 256)
        inside = (e[0] >= thr[0][gt]) & (e[1] >= thr[1][gt]) & (e[2] >= thr[2][gt])
        m = np.nonzero(inside)[0]
        gm = gt[m]
        wf = _inv_depth(e[1][m], e[2][m], (s * area[gt])[m], w[f[gm, 0]], w[f[gm, 1]], w[f[gm, 2]])
        pos = wf > 0
        key = (wf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - tri[gm].astype(np.uint64))
        np.maximum.at(keys, (pj[m] * W + pi[m])[pos], key[pos])
    return keys.reshape(H, W)


def resolve_host(keys, verts, faces, colors, X, Y, w, R, bgcolor, shade='color'):
    """Resolve pass: the four outputs from the visibility buffer."""
    H, W = keys.shape
    v = _np(verts, np.float32).reshape(-1, 3)
    f = _np(faces, np.int64).reshape(-1, 3)
    R = np.asarray(R, np.float32)
    flat = keys.reshape(-1)
    cov = np.nonzero(flat)[0]
    tri_id = np.full(H * W, -1, dtype=np.int32)
    depth = np.zeros(H * W, dtype=np.float32)
    alpha = np.zeros(H * W, dtype=np.float32)
    rgb = np.empty((H * W, 3), dtype=np.float32)
    rgb[:] = np.asarray(bgcolor, np.float32).reshape(3)
    t = (np.uint64(0xFFFFFFFF) - (flat[cov] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    wf = (flat[cov] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    tri_id[cov] = t.astype(np.int32)
    alpha[cov] = 1.0
    depth[cov] = np.float32(1.0) / wf
    ft = f[t]
    if shade == 'normal':
        with np.errstate(all='ignore'):
            a, b = v[ft[:, 1]] - v[ft[:, 0]], v[ft[:, 2]] - v[ft[:, 0]]
            c = [a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                 a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]]
            ln = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
            good = (ln > 0) & np.isfinite(ln)
            m = [np.where(good, ci / np.where(good, ln, np.float32(1)), np.float32(0)) for ci in c]
            for i in range(3):
                rgb[cov, i] = np.float32(0.5) + np.float32(0.5) * ((R[i, 0] * m[0] + R[i, 1] * m[1]) + R[i, 2] * m[2])
    else:
        col = _np(colors, np.float32).reshape(-1, 3)
        Pt = [(X[ft[:, c]], Y[ft[:, c]]) for c in range(3)]
        area = (Pt[1][0] - Pt[0][0]) * (Pt[2][1] - Pt[0][1]) - (Pt[1][1] - Pt[0][1]) * (Pt[2][0] - Pt[0][0])
        s = np.sign(area)
        e = _edges(Pt, s, (cov % W) * 256, (cov // W) * 256)
        A = (s * area).astype(np.float64)
        q = [e[c].astype(np.float64) / A * w[ft[:, c]].astype(np.float64) for c in range(3)]
        den = (q[0] + q[1]) + q[2]
        for i in range(3):
            cc = [col[ft[:, c], i].astype(np.float64) for c in range(3)]
            rgb[cov, i] = (((q[0] * cc[0] + q[1] * cc[1]) + q[2] * cc[2]) / den).astype(np.float32)
    return {'rgb': rgb.reshape(H, W, 3), 'alpha': alpha.reshape(H, W), 'depth': depth.reshape(H, W),
            'tri_id': tri_id.reshape(H, W)}


def rasterize_host(verts, faces, colors, K, E, H, W, bgcolor=(0, 0, 0), cull='none', shade='color', z_near=1e-3):
    """The rasteriser in numpy (module docstring): numpy outputs rgb (H, W, 3), alpha, depth (H, W) float32 and
    tri_id (H, W) int32, equal to ``rasterize``'s bit for bit.  ``colors`` may be None with ``shade='normal'``."""
    v = _np(verts, np.float32).reshape(-1, 3)
    f = _np(faces, np.int64).reshape(-1, 3)
    col = None if colors is None else _np(colors, np.float32).reshape(-1, 3)
    K, E = _np(K, np.float32), _np(E, np.float32)
    H, W = int(H), int(W)
    _check(v, f, col, K, E, H, W, cull, shade, z_near)
    X, Y, w, ok = project_host(v, K, E, z_near)
    keys = visibility_host(X, Y, w, ok, f, H, W, cull, camera_flips(K, E[:3, :3]))
    return resolve_host(keys, v, f, col, X, Y, w, E[:3, :3], bgcolor, shade)


def rasterize(verts, faces, colors, K, E, H, W, bgcolor=(0, 0, 0), cull='none', shade='color', z_near=1e-3):
    """The rasteriser on the device (hnrf_raster_mesh).  verts (V, 3) fp32, faces (F, 3) int32, colors (V, 3) fp32 in
    [0, 1] (None with ``shade='normal'``): tensors on the GPU; K (3, 3), E (4, 4), bgcolor (3,) in 0..1: host arrays or
    tensors.  Returns device tensors rgb (H, W, 3), alpha (H, W), depth (H, W), tri_id (H, W) int32.  Nothing here
    waits for the device."""
    import torch
    from . import _lib, ops
    if not (torch.is_tensor(verts) and verts.is_cuda):
        raise _lib.HnrfError('rasterize: verts must be a tensor on the GPU (rasterize_host is the numpy route)')
    dev = verts.device
    verts = verts.to(torch.float32).contiguous()
    faces = torch.as_tensor(faces).to(device=dev, dtype=torch.int32).contiguous()
    if colors is not None:
        colors = torch.as_tensor(colors).to(device=dev, dtype=torch.float32).contiguous()
    K, E = _np(K, np.float32), _np(E, np.float32)
    H, W = int(H), int(W)
    _check(verts, faces, colors, K, E, H, W, cull, shade, z_near)
    cam = np.concatenate([K.reshape(-1), E[:3, :3].reshape(-1), E[:3, 3].reshape(-1),
                          np.asarray(bgcolor, np.float32).reshape(3)]).astype(np.float32)
    return ops.raster_mesh(verts, faces, colors, ops._upload(cam, dev), H, W, float(np.float32(z_near)),
                           CULL[cull] | SHADE[shade])
