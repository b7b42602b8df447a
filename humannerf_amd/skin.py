"""Bone weights as data, and the skinning a glTF viewer performs with them (include/hnrf_skin.h).

``hnrf_forward_skin`` blends a canonical vertex over all B bones of the weight volume and keeps none of the weights.  A
skinned mesh file wants them as data: at most 4 (or 8) influences per vertex, normalised.  ``skin_weights`` samples the
weights exactly as forward skinning does (the same device function), keeps the K largest and normalises them;
``skin_lbs`` is the sum a viewer forms from them, ``sum_k weights[k] (mats[joints[k]] (x, 1))``, so that what the
truncation to K costs against the exact forward skin can be measured on the device (run.run_gltf does, per frame).

``skin_weights_host`` / ``skin_lbs_host`` restate the two kernels in numpy float32 operation for operation -- every
operation rounded on its own, in the order the header states -- and equal them bit for bit (the host / device idiom of
``mesh`` and ``baked``).  The conventions, in short:

- the weight of bone b is trilinear, align_corners, zero padding, summed over the corners k = 0..7 (x fastest) from 0;
  a NaN coordinate samples as zero-padded;
- the K largest POSITIVE weights, descending, equal weights in ascending bone order; unused slots are (joint 0,
  weight 0);
- ``kept`` = the fp32 sum of the selected weights in output order, ``weights[k] = w_k / kept``; ``kept == 0`` gives
  joints all 0 and weights (1, 0, ..., 0);
- ``joint_matrices`` turns a frame's motion basis (network.motion_basis: canonical <- observation) into the matrices
  ``skin_lbs`` and a viewer multiply by: the inverse of every bone's rigid transform, ``world(joint b) x
  inverseBind(b)`` in glTF's words.

The non-rigid offsets are no part of any of this: like hnrf_forward_skin, skinning poses the canonical surface.
"""
import numpy as np

_f = np.float32


def _k_of(k):
    k = int(k)
    if k not in (4, 8):
        raise ValueError('%d influences per vertex: glTF skinning is built for 4 or 8' % k)
    return k


def _n_bones(vol, n_bones):
    """The bone channels of a weight volume: all but the last (the background), as everywhere in this package."""
    B = vol.shape[0] - 1 if n_bones is None else int(n_bones)
    if not 1 <= B <= min(128, vol.shape[0]):
        raise ValueError('%d bones of a volume with %d channels (1 <= bones <= 128)' % (B, vol.shape[0]))
    return B


# ------------------------------------------------------------------------------------------------------ device
def skin_weights(verts, vol, bbox_min, bbox_scale, k=4, n_bones=None):
    """hnrf_skin_weights on CUDA tensors: verts (V, 3), vol (C, G, G, G), the canonical bbox as hnrf_forward_skin takes
    it.  ``n_bones``: how many leading channels are bones (None: C - 1, the last being the background).  Returns
    (joints (V, k) uint8, weights (V, k) fp32, kept (V,) fp32) on the device."""
    from . import ops
    return ops.skin_weights(verts, vol, _n_bones(vol, n_bones), bbox_min, bbox_scale, _k_of(k))


def skin_lbs(verts, joints, weights, mats):
    """hnrf_skin_lbs on CUDA tensors: verts (V, 3), joints (V, k) uint8, weights (V, k), mats (B, 3, 4) -> (V, 3)."""
    from . import ops
    return ops.skin_lbs(verts, joints, weights, mats)


def joint_matrices(motion_Rs, motion_Ts):
    """The inverse of every bone's rigid motion basis A_b(x) = R_b x + T_b as (B, 3, 4) float32 = [R_b^-1 | -R_b^-1
    T_b], computed in float64 (adjugate over determinant, no library call and nothing read back) and rounded once.
    Torch tensors give a tensor on their device, anything else a numpy array."""
    if hasattr(motion_Rs, 'detach'):
        import torch as xp
        R, T = motion_Rs.detach().to(xp.float64), motion_Ts.detach().to(xp.float64)
        done = lambda m: m.to(xp.float32).contiguous()
    else:
        xp = np
        R, T = np.asarray(motion_Rs, dtype=np.float64), np.asarray(motion_Ts, dtype=np.float64)
        done = lambda m: np.ascontiguousarray(m.astype(np.float32))
    r = lambda i, j: R[:, i, j]
    cof = [[r(1, 1) * r(2, 2) - r(1, 2) * r(2, 1), r(0, 2) * r(2, 1) - r(0, 1) * r(2, 2), r(0, 1) * r(1, 2) - r(0, 2) * r(1, 1)],
           [r(1, 2) * r(2, 0) - r(1, 0) * r(2, 2), r(0, 0) * r(2, 2) - r(0, 2) * r(2, 0), r(0, 2) * r(1, 0) - r(0, 0) * r(1, 2)],
           [r(1, 0) * r(2, 1) - r(1, 1) * r(2, 0), r(0, 1) * r(2, 0) - r(0, 0) * r(2, 1), r(0, 0) * r(1, 1) - r(0, 1) * r(1, 0)]]
    det = r(0, 0) * cof[0][0] + r(0, 1) * cof[1][0] + r(0, 2) * cof[2][0]
    rows = []
    for i in range(3):
        inv = [cof[i][j] / det for j in range(3)]
        rows.append(xp.stack(inv + [-(inv[0] * T[:, 0] + inv[1] * T[:, 1] + inv[2] * T[:, 2])], -1))
    return done(xp.stack(rows, 1))


# ------------------------------------------------------------------------------------------------------ numpy twins
def _host(a):
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _trilinear_host(verts, bbox_min, bbox_scale, G):
    """trilinear_at of csrc/hnrf_trilinear.h for every vertex: corner offsets (V, 8) int64 and weights (V, 8) fp32."""
    gm1 = _f(G - 1)
    u, c = [], []
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(3):
            i = (((verts[:, a] - bbox_min[a]) * bbox_scale[a] - _f(1)) + _f(1)) * _f(0.5) * gm1
            f0 = np.floor(i)
            w1, w0 = i - f0, (f0 + _f(1)) - i
            x0 = np.fmin(np.fmax(f0, _f(-2)), gm1 + _f(1)).astype(np.int64)         # (fmaxf(NaN, -2) = -2)
            u.append((np.where((x0 >= 0) & (x0 < G), w0, _f(0)), np.where((x0 + 1 >= 0) & (x0 + 1 < G), w1, _f(0))))
            c.append((np.clip(x0, 0, G - 1), np.clip(x0 + 1, 0, G - 1)))
        off = np.empty((len(verts), 8), np.int64)
        cw = np.empty((len(verts), 8), np.float32)
        for k in range(8):
            dx, dy, dz = k & 1, (k >> 1) & 1, (k >> 2) & 1
            off[:, k] = c[2][dz] * (G * G) + c[1][dy] * G + c[0][dx]
            cw[:, k] = u[0][dx] * u[1][dy] * u[2][dz]
    return off, cw


def bone_weights_host(verts, vol, bbox_min, bbox_scale, n_bones=None):
    """The weights hnrf_forward_skin blends with, (V, B) float32, bit for bit: w = 0, then w = w + vol[b][corner k] *
    c_k for k = 0..7."""
    verts, vol, bmin, bscale = _host(verts).reshape(-1, 3), _host(vol), _host(bbox_min).reshape(3), _host(bbox_scale).reshape(3)
    B, G = _n_bones(vol, n_bones), vol.shape[-1]
    off, cw = _trilinear_host(verts, bmin, bscale, G)
    flat = vol[:B].reshape(B, -1)
    w = np.zeros((len(verts), B), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(8):
            w = w + flat[:, off[:, k]].T * cw[:, k, None]
    return w


def skin_weights_host(verts, vol, bbox_min, bbox_scale, k=4, n_bones=None):
    """hnrf_skin_weights in numpy float32: (joints (V, k) uint8, weights (V, k) float32, kept (V,) float32), equal to
    the kernel's bit for bit."""
    K = _k_of(k)
    w = bone_weights_host(verts, vol, bbox_min, bbox_scale, n_bones)
    V, B = w.shape
    s = np.zeros((V, K), np.float32)
    j = np.zeros((V, K), np.int64)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for b in range(B):
            cw, cj = w[:, b].copy(), np.full(V, b, np.int64)
            moved = np.zeros(V, bool)
            for q in range(K):
                ins = moved | (cw > s[:, q])
                ts, tj = s[:, q].copy(), j[:, q].copy()
                s[:, q], j[:, q] = np.where(ins, cw, ts), np.where(ins, cj, tj)
                cw, cj, moved = np.where(ins, ts, cw), np.where(ins, tj, cj), ins
        kept = s[:, 0].copy()
        for q in range(1, K):
            kept = kept + s[:, q]
        ok = kept > 0
        unit = np.zeros((V, K), np.float32)
        unit[:, 0] = 1
        weights = np.where(ok[:, None], s / np.where(ok, kept, _f(1))[:, None], unit).astype(np.float32)
    joints = np.where(ok[:, None], j, 0).astype(np.uint8)
    return joints, weights, kept


def skin_lbs_host(verts, joints, weights, mats):
    """hnrf_skin_lbs in numpy float32, bit for bit: acc = 0; for k in order, p_i = ((m_i0 x + m_i1 y) + m_i2 z) + m_i3
    with m = mats[joints[k]], acc_i = acc_i + weights[k] p_i; a slot whose joint is >= B is skipped."""
    verts, weights, mats = _host(verts).reshape(-1, 3), _host(weights), _host(mats)
    joints = np.asarray(joints.detach().cpu().numpy() if hasattr(joints, 'detach') else joints).astype(np.int64)
    K, B = _k_of(weights.shape[-1]), mats.shape[0]
    x, y, z = verts[:, 0, None], verts[:, 1, None], verts[:, 2, None]
    acc = np.zeros((len(verts), 3), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for q in range(K):
            valid = joints[:, q] < B
            m = mats[np.minimum(joints[:, q], B - 1)]                                # (V, 3, 4)
            p = ((m[:, :, 0] * x + m[:, :, 1] * y) + m[:, :, 2] * z) + m[:, :, 3]
            acc = np.where(valid[:, None], acc + weights[:, q, None] * p, acc)
    return acc
