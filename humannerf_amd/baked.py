"""Baked canonical grid: the canonical MLP tabulated on an N^3 lattice (hnrf_bake_canonical) and looked up by
trilinear interpolation (hnrf_baked_sample) where the volume renderer would run the MLP -- an opt-in approximation
(``cfg.amd.canonical = 'baked'``), include/hnrf.h "baked canonical grid".

This module is the host side: ``sample_host`` restates the device sampler in numpy float32, bit for bit (the
host/device idiom of ``mesh`` and ``imageproc``); ``lattice_points`` are the positions the bake evaluates;
``save_grid`` / ``load_grid`` ship a baked avatar without re-baking.  ``warp_sample_host`` is the twin of the fused
sampler of the per-frame offset grid (``cfg.amd.nonrigid = 'baked'``, hnrf_bake_nonrigid / hnrf_baked_warp_sample): a
grid of the same layout with c = (dx, dy, dz, +0).  The conventions:

- ``grid`` (N, N, N, 4) float16 indexed [z][y][x][c], c = (r, g, b, sigma) pre-activation, 8 <= N <= 512, on the
  lattice of ``mesh.lattice_axes``;
- per axis, in float32 with n = N - 1: ``inv_step = n / (bbox_max - bbox_min)``, ``u = (x - bbox_min) * inv_step``
  clamped to [0, n] (border replicate; a NaN coordinate samples index 0), ``i0 = min(floor(u), n - 1)``,
  ``t = u - i0``;
- blend ``a + t * (b - a)`` along x, then y, then z, every operation rounded on its own.
"""
import hashlib

import numpy as np

from .mesh import lattice_axes

N_MIN, N_MAX = 8, 512


def check_resolution(N):
    N = int(N)
    if not N_MIN <= N <= N_MAX:
        raise ValueError('baked grid resolution %d out of range [%d, %d]' % (N, N_MIN, N_MAX))
    return N


def lattice_points(bbox_min, bbox_max, N):
    """float32 (N^3, 3): the lattice positions in grid order ([z][y][x], x fastest), as the bake computes them."""
    ax = lattice_axes(bbox_min, bbox_max, check_resolution(N))
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    return np.stack([x, y, z], -1).reshape(-1, 3)


def _axis(x, lo, hi, N):
    n = np.float32(N - 1)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        inv_step = n / (hi - lo)
        u = (x - lo) * inv_step
    u = np.fmin(np.fmax(u, np.float32(0.0)), n)            # fmax(NaN, 0) = 0, as the device's
    i0 = np.minimum(np.floor(u).astype(np.int64), N - 2)
    return i0, u - i0.astype(np.float32)


def sample_host(grid, xyz, bbox_min, bbox_max):
    """The device sampler in numpy float32: grid (N, N, N, 4) float16, xyz (..., 3) -> raw (..., 4) float32."""
    grid = np.asarray(grid)
    N = check_resolution(grid.shape[0])
    if grid.shape != (N, N, N, 4) or grid.dtype != np.float16:
        raise ValueError('grid must be float16 (N, N, N, 4), got %s %s' % (grid.dtype, grid.shape))
    xyz = np.asarray(xyz, dtype=np.float32)
    lead = xyz.shape[:-1]
    p = xyz.reshape(-1, 3)
    lo = np.asarray(bbox_min, dtype=np.float32).reshape(3)
    hi = np.asarray(bbox_max, dtype=np.float32).reshape(3)
    (ix, tx), (iy, ty), (iz, tz) = (_axis(p[:, a], lo[a], hi[a], N) for a in range(3))
    tx, ty, tz = tx[:, None], ty[:, None], tz[:, None]
    with np.errstate(invalid='ignore', over='ignore'):
        d = []
        for dz in (0, 1):
            e = []
            for dy in (0, 1):
                a = grid[iz + dz, iy + dy, ix].astype(np.float32)
                b = grid[iz + dz, iy + dy, ix + 1].astype(np.float32)
                e.append(a + tx * (b - a))
            d.append(e[0] + ty * (e[1] - e[0]))
        out = d[0] + tz * (d[1] - d[0])
    return out.astype(np.float32).reshape(lead + (4,))


def warp_sample_host(off_grid, cnl_grid, x_skel, boxes):
    """The fused device sampler (hnrf_baked_warp_sample) in numpy float32: ``off = sample_host(off_grid, x_skel)[:3]``,
    ``xyz = x_skel + off`` (one float32 add per coordinate), ``raw = sample_host(cnl_grid, xyz)``.  ``boxes`` =
    ((off_bbox_min, off_bbox_max), (cnl_bbox_min, cnl_bbox_max)), or one (bbox_min, bbox_max) pair for both grids.
    x_skel (..., 3) -> (raw (..., 4), xyz (..., 3), offsets (..., 3)), all float32."""
    boxes = tuple(boxes)
    if len(boxes) == 2 and np.ndim(boxes[0][0]) == 0:
        boxes = (boxes, boxes)
    (olo, ohi), (clo, chi) = boxes
    x_skel = np.asarray(x_skel, dtype=np.float32)
    off = sample_host(off_grid, x_skel, olo, ohi)[..., :3]
    with np.errstate(invalid='ignore', over='ignore'):
        xyz = (x_skel + off).astype(np.float32)
    return sample_host(cnl_grid, xyz, clo, chi), xyz, np.ascontiguousarray(off)


def weights_hash(tensors):
    """sha256 over the float32 bytes of the canonical MLP's weights and biases (torch tensors or arrays, in the order
    of pts_linears.{0..14}, output_linear.0; weight then bias per layer)."""
    h = hashlib.sha256()
    for t in tensors:
        a = t.detach().cpu().numpy() if hasattr(t, 'detach') else np.asarray(t)
        h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return h.hexdigest()


def save_grid(path, grid, bbox_min, bbox_max, mode, weights_hash=None):
    """Write a baked grid as .npz: grid (float16 bits), bbox_min / bbox_max, N, mode, and the hash of the canonical
    weights it was baked from ('' when unknown)."""
    g = grid.detach().cpu().numpy() if hasattr(grid, 'detach') else np.asarray(grid)
    N = check_resolution(g.shape[0])
    if g.shape != (N, N, N, 4) or g.dtype != np.float16:
        raise ValueError('grid must be float16 (N, N, N, 4), got %s %s' % (g.dtype, g.shape))
    host = lambda a: (a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)).astype(np.float32).reshape(3)
    with open(path, 'wb') as f:
        np.savez(f, grid=np.ascontiguousarray(g).view(np.uint16), bbox_min=host(bbox_min), bbox_max=host(bbox_max),
                 N=np.int64(N), mode=np.str_(mode), weights_hash=np.str_(weights_hash or ''))


def load_grid(path):
    """-> dict(grid float16 (N, N, N, 4), bbox_min, bbox_max float32 (3,), N, mode, weights_hash or None)."""
    with np.load(path, allow_pickle=False) as z:
        grid = np.ascontiguousarray(z['grid']).view(np.float16)
        N = int(z['N'])
        if grid.shape != (N, N, N, 4):
            raise ValueError('%s: grid %s does not match N = %d' % (path, grid.shape, N))
        return {'grid': grid, 'bbox_min': z['bbox_min'].astype(np.float32), 'bbox_max': z['bbox_max'].astype(np.float32),
                'N': N, 'mode': str(z['mode']), 'weights_hash': str(z['weights_hash']) or None}
