"""The predicate of cfg.amd.share_underflow in numpy float32: the twin of hnrf_share_compact's classification
(include/hnrf.h states the predicate; humannerf_amd/csrc/hnrf_sample_warp.hip evaluates it on the device).

A sample is SHARED -- its non-rigid offset, canonical position and raw are those of the frame's representative
x_skel = (+0, +0, +0) bit for bit in 'f16x3' mode -- when for every axis a
  (a) |x_skel[a]| <= SHARE_T = 2^-31, and
  (b) the bits of the fp32 sum x_skel[a] + c_off[a] equal the bits of c_xyz[a],
with c_off / c_xyz the offsets / xyz the non-rigid kernel wrote for the representative.  NaN and infinite
coordinates fail (a): such samples are always live."""
import numpy as np

SHARE_T = np.float32(2.0 ** -31)


def shared_mask(x_skel, c_off, c_xyz):
    """x_skel (..., 3), c_off (3,), c_xyz (3,) -> bool (...): True where the sample is shared.  IEEE fp32 arithmetic
    with subnormals, as the kernels run."""
    x = np.asarray(x_skel, dtype=np.float32)
    c_off = np.asarray(c_off, dtype=np.float32).reshape(3)
    c_xyz = np.asarray(c_xyz, dtype=np.float32).reshape(3)
    with np.errstate(invalid='ignore', over='ignore'):
        small = np.abs(x) <= SHARE_T                              # False for NaN
        s = (x + c_off).astype(np.float32)
    same = s.view(np.uint32) == c_xyz.view(np.uint32)
    return np.logical_and(small, same).all(axis=-1)


def live_indices(x_skel, c_off, c_xyz):
    """Sorted flat indices of the samples the MLPs still evaluate (the device list holds the same set, in block order)."""
    return np.flatnonzero(~shared_mask(np.asarray(x_skel, dtype=np.float32).reshape(-1, 3), c_off, c_xyz))


def fill_planes(x_skel, c_off, c_xyz, c_raw, planes):
    """The twin of hnrf_share_compact_heads (include/hnrf_heads_shared.h): ``planes`` (H, P, 4) float32, written in
    place -- row p of plane g becomes c_raw[g] (H, 4) where sample p is shared, and no row of a live sample is touched
    in any plane.  Returns the live list (sorted; each live sample once, whatever H is)."""
    c_raw = np.asarray(c_raw, dtype=np.float32)
    H, P = planes.shape[:2]
    if planes.dtype != np.float32 or planes.shape != (H, P, 4) or c_raw.shape != (H, 4):
        raise ValueError('fill_planes: planes (H, P, 4) float32 and c_raw (H, 4), got %s %s and %s'
                         % (planes.dtype, planes.shape, c_raw.shape))
    m = shared_mask(np.asarray(x_skel, dtype=np.float32).reshape(P, 3), c_off, c_xyz)
    for g in range(H):
        planes[g, m] = c_raw[g]
    return np.flatnonzero(~m)
