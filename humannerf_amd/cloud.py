"""Surface-point records and the frame x frame appearance distance: the reference's ``cfg.test.save_3d_together``
dump (run.py:388-404, image_util.py:99-119) and ``tools/compute_distance*.py`` on this package's kernels
(include/hnrf_cloud.h, csrc/hnrf_cloud.hip).

  surface_records   one record per ray whose largest weight passes the threshold: [N, 10] fp32 on the device, the
                    reference's columns -- weighted xyz (3) | image rgb (3) | weight max | pixel row, col | lbs argmax
  nearest_pairs     find_nearest_pair_gpu: the mutual nearest neighbours of two clouds
  frame_distance    compute_distance_gpu: the summed colour error of the mutual pairs closer than dist_thresh
  distance_matrix   the frame x frame matrix of the tools' main loop, all pairs of a chunk in one launch
  segment_records   tools/segment.py: a frame's records split by body part (include/hnrf_segment.h, csrc/hnrf_segment.hip;
                    integer arithmetic, twin_segment / twin_compact are the numpy form, bit for bit)
  segment_distance_matrices   the per-part matrices of tools/compute_distance_seg.py, all parts from one pack
  cluster_frames, merge_matrix_chunks   tools/cluster.py and tools/merge_d.py, numpy on the host

The arithmetic is one statement (hnrf_cloud.h): d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) in fp32, nearest =
smallest d2 with ties to the lowest original record index, distance = fl(sqrt(d2)).  The ``twin_*`` functions below are
its numpy form, brute force and windowed; the kernels equal them bit for bit (tests/test_gpu_cloud.py), and
``backend='twin'`` runs the public functions through them without a GPU (slow: for tests and for checking a kernel
result, never chosen silently).
"""
import numpy as np

from ._lib import HnrfError

RECORD_KEYS = ('weights_on_rays', 'xyz_on_rays', 'backward_motion_weights')
WINDOW_SLACK = 1.0 + 2.0 ** -20          # the window is |dk| <= tau (1 + 2^-20), formed in fp64


# ------------------------------------------------------------------------------------------------ the numpy twin
def _f32(x, cols=3):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, cols))


def twin_d2(a, b):
    """d2 of the statement on fp32 arrays (..., 3), broadcasting.  numpy rounds every operation: no contraction."""
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _argmin_by_orig(d2, orig):
    """Row-wise argmin of d2 (n, m), ties to the smallest ``orig`` (m,)."""
    best = d2.min(axis=1)
    cand = np.where(d2 == best[:, None], orig[None, :].astype(np.int64), np.int64(1) << 40)
    return cand.argmin(axis=1).astype(np.int64), best


def twin_nn(a, b, orig=None):
    """Brute force: for every a the position in b of its nearest neighbour and its d2; ties to the lowest ``orig``
    (default: the position itself).  An empty b gives -1 / +inf."""
    a, b = _f32(a), _f32(b)
    if b.shape[0] == 0 or a.shape[0] == 0:
        return np.full(a.shape[0], -1, np.int64), np.full(a.shape[0], np.inf, np.float32)
    orig = np.arange(b.shape[0]) if orig is None else np.asarray(orig)
    pos, best = np.empty(a.shape[0], np.int64), np.empty(a.shape[0], np.float32)
    for s in range(0, a.shape[0], 512):
        pos[s:s + 512], best[s:s + 512] = _argmin_by_orig(twin_d2(a[s:s + 512, None, :], b[None, :, :]), orig)
    return pos, best


def twin_window_nn(a, b, orig, axis, tau):
    """The windowed search: b sorted ascending along ``axis``; per a the argmin of d2 over the b with
    |k_a - k_b| <= tau (1 + 2^-20) (fp64 bounds), ties by ``orig``.  An empty window gives -1 / +inf."""
    a, b, orig = _f32(a), _f32(b), np.asarray(orig)
    keys = b[:, axis].astype(np.float64)
    win = np.float64(np.float32(tau)) * WINDOW_SLACK
    ka = a[:, axis].astype(np.float64)
    first = np.searchsorted(keys, ka - win, side='left')
    last = np.searchsorted(keys, ka + win, side='right')
    pos, best = np.full(a.shape[0], -1, np.int64), np.full(a.shape[0], np.inf, np.float32)
    for i in np.nonzero(last > first)[0]:
        p, d = _argmin_by_orig(twin_d2(a[i:i + 1, None, :], b[None, first[i]:last[i], :]), orig[first[i]:last[i]])
        if not np.isnan(d[0]):
            pos[i], best[i] = first[i] + p[0], d[0]
    return pos, best


def sort_frame(xyz, rgb, axis):
    """A frame as the pair kernel wants it: rows sorted ascending by coordinate ``axis``, ``orig`` = the record index."""
    xyz, rgb = _f32(xyz), _f32(rgb)
    order = np.argsort(xyz[:, axis], kind='stable')
    return {'xyz': xyz[order], 'rgb': rgb[order], 'orig': order.astype(np.int32)}


def twin_pairs(fi, fj, tau, axis, method='window'):
    """One pair of sorted frames (sort_frame) -> (match, err, D): per sorted position of frame i the partner's orig or
    -1, the pair's colour error in fp32 (0 without partner), and D = the fp64 sum of err in position order."""
    tau = np.float32(tau)
    search = (lambda a, f: twin_window_nn(a, f['xyz'], f['orig'], axis, tau)) if method == 'window' else \
             (lambda a, f: twin_nn(a, f['xyz'], f['orig']))
    ni = fi['xyz'].shape[0]
    match, err = np.full(ni, -1, np.int32), np.zeros(ni, np.float32)
    q, d2 = search(fi['xyz'], fj)
    near = (q >= 0) & (np.sqrt(d2) < tau)
    p = np.nonzero(near)[0]
    if p.size:
        back, _ = search(fj['xyz'][q[p]], fi)
        p = p[back == p]
        match[p] = fj['orig'][q[p]]
        err[p] = np.sqrt(twin_d2(fi['rgb'][p], fj['rgb'][q[p]]))
    return match, err, float(np.sum(err.astype(np.float64))) if ni else 0.0


def twin_nearest_pairs(x0, x1):
    """find_nearest_pair_gpu in the statement's arithmetic: (pair_0, pair_1, d01, d10)."""
    x0, x1 = _f32(x0), _f32(x1)
    m0, d01 = twin_nn(x0, x1)
    m1, d10 = twin_nn(x1, x0)
    if x0.shape[0] == 0 or x1.shape[0] == 0:
        e = np.zeros(0, np.int64)
        return e, e, np.sqrt(d01), np.sqrt(d10)
    pair_0 = np.nonzero(m1[m0] == np.arange(x0.shape[0]))[0]
    return pair_0, m0[pair_0], np.sqrt(d01), np.sqrt(d10)


def twin_surface_points(weights, xyz, bmw):
    """hnrf_surface_points in numpy, sum for sum: lane l of 64 adds the samples l, l + 64, ... ascending in fp32, then
    the butterfly over the lane distances 32 .. 1.  weights (R, S), xyz (R, S, 3), bmw (R, S, B) -> wxyz, wmax, lbs."""
    w = np.asarray(weights, dtype=np.float32)
    R, S = w.shape
    cols = np.concatenate([np.asarray(xyz, np.float32).reshape(R, S, 3), np.asarray(bmw, np.float32).reshape(R, S, -1)], 2)
    acc = np.zeros((R, 64, cols.shape[2]), np.float32)
    for s0 in range(0, S, 64):
        n = min(64, S - s0)
        acc[:, :n] = acc[:, :n] + w[:, s0:s0 + n, None] * cols[:, s0:s0 + n]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off]
    return acc[:, 0, :3].copy(), w.max(axis=1), acc[:, 0, 3:].argmax(axis=1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ records
def surface_records(out, truth, ray_index, width, weight_threshold, backend='hip'):
    """run.py:390-404 on the outputs of one forward: ``out`` must hold the diagnostic keys (cfg.amd.diagnostics),
    ``truth`` (R, 3) the image colours under the rays, ``ray_index`` (R,) the flat pixel index of every ray.  Returns
    the device tensor [N, 10] of the rays with weight max > ``weight_threshold``, in ray order (``backend='twin'``:
    twin_surface_points on host copies, a CPU tensor)."""
    import torch
    from . import ops
    missing = [k for k in RECORD_KEYS if k not in out]
    if missing:
        raise HnrfError('surface_records: the forward returned no %s: the records need the per-sample outputs, '
                        'set cfg.amd.diagnostics = True' % ', '.join(missing))
    w = out['weights_on_rays']
    R = w.shape[0]
    if truth is None or tuple(truth.shape) != (R, 3) or ray_index.numel() != R:
        raise HnrfError('surface_records: truth (R, 3) and ray_index (R,) must match the %d rays' % R)
    if backend == 'twin':
        w = w.detach().cpu()
        wxyz, wmax, lbs = (torch.from_numpy(v) for v in twin_surface_points(
            w.numpy(), _host(out['xyz_on_rays']), _host(out['backward_motion_weights'])))
    else:
        wxyz, wmax, lbs = ops.surface_points(w.contiguous(), out['xyz_on_rays'].contiguous(),
                                             out['backward_motion_weights'].contiguous())
    ray_index = ray_index.reshape(-1).to(w.device)
    row, col = torch.div(ray_index, int(width), rounding_mode='floor'), ray_index % int(width)
    rec = torch.cat([wxyz, truth.to(w.device, torch.float32), wmax[:, None], row[:, None].float(), col[:, None].float(),
                     lbs[:, None].float()], dim=1)
    return rec[wmax > float(weight_threshold)]


def _device(device):
    import torch
    dev = torch.device('cuda' if device is None else device)
    if dev.type != 'cuda' or not torch.cuda.is_available():
        raise HnrfError("the cloud kernels need a GPU (device %s); backend='twin' is the numpy statement" % dev)
    return dev


def _dev32(x, dev):
    import torch
    return torch.as_tensor(x).to(dev, torch.float32).reshape(-1, 3).contiguous()


def nearest_pairs(x0, x1, dist_thresh=None, backend='hip', device=None):
    """find_nearest_pair_gpu: (pair_0, pair_1, d01, d10), all 1-D -- the indices into x0 of the points that are the
    nearest neighbour of their nearest neighbour, their partners in x1, and every point's distance to its nearest
    neighbour (d01 per point of x0, d10 per point of x1), from two hnrf_cloud_nn launches.  With ``dist_thresh`` the
    windowed kernel decides instead: only the pairs closer than it are returned, and d01 / d10 are None."""
    import torch
    from . import ops
    if backend == 'twin':
        if dist_thresh is None:
            return twin_nearest_pairs(x0, x1)
        f0, f1 = sort_frame(x0, x0, 0), sort_frame(x1, x1, 0)
        match = twin_pairs(f0, f1, dist_thresh, 0)[0]
        keep = match >= 0
        o = np.argsort(f0['orig'][keep])
        return f0['orig'][keep][o].astype(np.int64), match[keep][o].astype(np.int64), None, None
    dev = _device(device if device is not None or not (torch.is_tensor(x0) and x0.is_cuda) else x0.device)
    a, b = _dev32(x0, dev), _dev32(x1, dev)
    if dist_thresh is None:
        m0, d01 = ops.cloud_nn(a, b)
        m1, d10 = ops.cloud_nn(b, a)
        if a.shape[0] == 0 or b.shape[0] == 0:
            e = torch.zeros(0, dtype=torch.int64, device=dev)
            return e, e, d01.sqrt(), d10.sqrt()
        pair_0 = torch.nonzero(m1[m0.long()] == torch.arange(a.shape[0], device=dev)).reshape(-1)
        return pair_0, m0[pair_0].long(), d01.sqrt(), d10.sqrt()
    pk = _pack([a, b], 0, dev)
    pairs = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    _, match = ops.cloud_distance_pairs(pk['xyz'], pk['rgb'], pk['orig'], pk['offsets'], pairs, dist_thresh, 0,
                                        pk['max_n'], want_match=True)
    match = match[0, :a.shape[0]]
    keep = match >= 0
    p0, p1 = pk['orig'][:a.shape[0]][keep].long(), match[keep].long()
    o = torch.argsort(p0)
    return p0[o], p1[o], None, None


def _pack(frames, axis, dev, colours=None):
    """Device frames (n, 3) -> the packed, per-frame sorted arrays of hnrf_cloud_distance_pairs (torch.sort per frame)."""
    import torch
    xyz, rgb, orig, counts = [], [], [], []
    for k, x in enumerate(frames):
        o = torch.sort(x[:, axis])[1]
        xyz.append(x[o])
        rgb.append((x if colours is None else colours[k])[o])
        orig.append(o.to(torch.int32))
        counts.append(x.shape[0])
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), device=dev)
    cat = lambda ts, shape, dt: torch.cat(ts).contiguous() if ts else torch.zeros(shape, dtype=dt, device=dev)
    return {'xyz': cat(xyz, (0, 3), torch.float32), 'rgb': cat(rgb, (0, 3), torch.float32),
            'orig': cat(orig, (0,), torch.int32), 'offsets': offsets, 'max_n': max(counts + [0])}


def _valid(rec, valid_weight_threshold):
    """compute_distance_gpu's filter on column 6 -> (xyz, rgb) of the kept rows, as the record's own tensor type."""
    keep = rec[:, 6] > valid_weight_threshold
    rec = rec[keep]
    return rec[:, 0:3], rec[:, 3:6]


def default_axis(clouds):
    """The coordinate of largest extent over all points of all frames (the narrowest windows); 0 without points."""
    pts = [np.asarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds if len(c)]
    if not pts:
        return 0
    lo = np.min([p.min(axis=0) for p in pts], axis=0)
    hi = np.max([p.max(axis=0) for p in pts], axis=0)
    return int(np.argmax(hi - lo))


def chunk_rows(F, chunk):
    """The rows of the matrix that chunk (chunk_id, chunk_n) computes: arange(chunk_id, F, chunk_n), and for the last
    chunk the reference's tail rule -- every row after its last one as well (compute_distance_seg.py:64-66)."""
    chunk_id, chunk_n = int(chunk[0]), int(chunk[1])
    if not (chunk_n >= 1 and 0 <= chunk_id < chunk_n):
        raise ValueError('chunk (id, n) must have 0 <= id < n, got %r' % (chunk,))
    idx = np.arange(chunk_id, F, chunk_n)
    if chunk_id == chunk_n - 1 and idx.size:
        idx = np.concatenate([idx, np.arange(idx[-1] + 1, F)])
    return idx


def matrix_file_name(valid_weight_threshold=0.3, dist_thresh=0.002, chunk=(0, 1)):
    """The reference's file name (its cluster.py reads it): distance_mat_{vwt:.2f}-{tau:.2f}[.{id}-{n}].npy."""
    name = 'distance_mat_%.2f-%.2f' % (valid_weight_threshold, dist_thresh)
    if tuple(chunk) != (0, 1):
        name += '.%d-%d' % (int(chunk[0]), int(chunk[1]))
    return name + '.npy'


def _host(t):
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else np.asarray(t)


def _brute_pair_hip(a, ca, b, cb, tau):
    """One pair by two hnrf_cloud_nn launches; the threshold and the colour errors on the host in the twin's arithmetic."""
    from . import ops
    if a.shape[0] == 0 or b.shape[0] == 0:
        return 0.0
    m0, d2 = ops.cloud_nn(a, b)
    m1, _ = ops.cloud_nn(b, a)
    m0, m1, d2 = _host(m0).astype(np.int64), _host(m1).astype(np.int64), _host(d2)
    p = np.nonzero((m1[m0] == np.arange(m0.size)) & (np.sqrt(d2) < np.float32(tau)))[0]
    err = np.sqrt(twin_d2(_host(ca)[p], _host(cb)[m0[p]]))
    return float(np.sum(err.astype(np.float64)))


def distance_matrix(records, valid_weight_threshold=0.3, dist_thresh=0.002, chunk=(0, 1), method='window', axis=None,
                    backend='hip', device=None, pairs_per_launch=1 << 16):
    """The main loop of tools/compute_distance*.py: ``records`` maps frame name -> [N, 10] record tensor (or None); the
    frames in sorted name order, each filtered on column 6 > ``valid_weight_threshold`` and sorted once along ``axis``
    (default: the axis of largest extent over all kept points); the rows of ``chunk`` = (chunk_id, chunk_n), i < j
    only, mirrored.  A None record gives 0.  ``method``: 'window' = hnrf_cloud_distance_pairs, every pair of the chunk
    in launches of ``pairs_per_launch``; 'brute' = hnrf_cloud_nn both ways per pair.  Both give the same pairs.
    Returns np.float32 [F, F] (the reference stores its fp32 sums in a float32 matrix)."""
    if method not in ('window', 'brute') or backend not in ('hip', 'twin'):
        raise ValueError("method must be 'window' or 'brute' and backend 'hip' or 'twin'")
    tau = float(dist_thresh)
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError('dist_thresh must be finite and > 0, got %r' % dist_thresh)
    names = sorted(records.keys())
    F = len(names)
    D = np.zeros((F, F), dtype=np.float32)
    have = [records[n] is not None for n in names]
    rows = chunk_rows(F, chunk)
    todo = [(i, j) for i in dict.fromkeys(rows.tolist()) for j in range(i + 1, F) if have[i] and have[j]]
    if not todo:
        return D
    if backend == 'twin':
        clouds = {k: tuple(_host(t) for t in _valid(records[names[k]], valid_weight_threshold))
                  for k in range(F) if have[k]}
        axis = default_axis([c[0] for c in clouds.values()]) if axis is None else int(axis)
        frames = {k: sort_frame(c[0], c[1], axis) for k, c in clouds.items()}
        for i, j in todo:
            D[i, j] = D[j, i] = twin_pairs(frames[i], frames[j], tau, axis, method)[2]
        return D
    import torch
    from . import ops
    dev = _device(device)
    empty = torch.zeros(0, 3, device=dev)
    xyz, rgb = [empty] * F, [empty] * F
    for k in range(F):
        if have[k]:
            x, c = _valid(torch.as_tensor(records[names[k]]).to(dev, torch.float32), valid_weight_threshold)
            xyz[k], rgb[k] = x.contiguous(), c.contiguous()
    if axis is None:
        ext = [torch.stack([x.min(0)[0], x.max(0)[0]]) for x in xyz if x.shape[0]]
        axis = 0 if not ext else int(torch.argmax(torch.stack([e[1] for e in ext]).max(0)[0]
                                                  - torch.stack([e[0] for e in ext]).min(0)[0]))
    if method == 'brute':
        for i, j in todo:
            D[i, j] = D[j, i] = _brute_pair_hip(xyz[i], rgb[i], xyz[j], rgb[j], tau)
        return D
    pk = _pack(xyz, int(axis), dev, colours=rgb)
    for s in range(0, len(todo), int(pairs_per_launch)):
        part = todo[s:s + int(pairs_per_launch)]
        pairs = torch.tensor(part, dtype=torch.int32, device=dev)
        d, _ = ops.cloud_distance_pairs(pk['xyz'], pk['rgb'], pk['orig'], pk['offsets'], pairs, tau, int(axis), pk['max_n'])
        for (i, j), v in zip(part, d.cpu().numpy()):
            D[i, j] = D[j, i] = v
    return D


def frame_distance(rec0, rec1, valid_weight_threshold=0.3, dist_thresh=0.002, method='window', axis=None,
                   backend='hip', device=None):
    """compute_distance_gpu of two records: 0 where either is None, else the summed colour error of their mutual
    nearest pairs closer than ``dist_thresh`` (float; the fp64 sum of the fp32 errors)."""
    if rec0 is None or rec1 is None:
        return 0
    recs = {'0': rec0, '1': rec1}
    return float(_pair_value(recs, valid_weight_threshold, dist_thresh, method, axis, backend, device))


def _pair_value(recs, vwt, tau, method, axis, backend, device):
    if backend == 'twin':                                               # (not through the float32 matrix)
        c = [tuple(_host(t) for t in _valid(recs[k], vwt)) for k in ('0', '1')]
        axis = default_axis([c[0][0], c[1][0]]) if axis is None else int(axis)
        return twin_pairs(sort_frame(c[0][0], c[0][1], axis), sort_frame(c[1][0], c[1][1], axis), tau, axis, method)[2]
    import torch
    from . import ops
    dev = _device(device)
    fr = [_valid(torch.as_tensor(recs[k]).to(dev, torch.float32), vwt) for k in ('0', '1')]
    if method == 'brute':
        return _brute_pair_hip(fr[0][0].contiguous(), fr[0][1], fr[1][0].contiguous(), fr[1][1], tau)
    axis = default_axis([_host(fr[0][0]), _host(fr[1][0])]) if axis is None else int(axis)
    pk = _pack([fr[0][0], fr[1][0]], axis, dev, colours=[fr[0][1], fr[1][1]])
    pairs = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    return float(ops.cloud_distance_pairs(pk['xyz'], pk['rgb'], pk['orig'], pk['offsets'], pairs, tau, axis,
                                          pk['max_n'])[0][0])


# ------------------------------------------------------------------------------------------------ body parts
# tools/segment.py:5-14 as data: part -> the bones (lbs arg-max) that seed it, in the reference's order
BODY_PARTS = {
    'root': (0,), 'lhip': (1,), 'rhip': (2,), 'lknee': (4,), 'rknee': (5,), 'lfoot': (7, 10), 'rfoot': (8, 11),
    'belly': (3,), 'spine': (6,), 'chest-inshoulder-neck': (9, 12, 13, 14), 'head': (15,),
    'lshoulder-elbow': (16, 18), 'rshoulder-elbow': (17, 19), 'lwrist-hand': (20, 22), 'rwrist-hand': (21, 23)}
MAX_PARTS, MAX_BONES, MAX_RADIUS = 32, 32, 64


def bone_masks(parts=None):
    """The per-bone uint32 words of hnrf_segment_members: bit p of word b set iff bone b seeds part p (parts in the
    mapping's order).  At most 32 parts; a bone outside [0, 32) can seed nothing and is refused."""
    parts = BODY_PARTS if parts is None else parts
    if not 1 <= len(parts) <= MAX_PARTS:
        raise ValueError('parts: 1 .. %d parts, got %d' % (MAX_PARTS, len(parts)))
    masks = np.zeros(MAX_BONES, np.uint32)
    for p, bones in enumerate(parts.values()):
        for b in bones:
            if int(b) != b or not 0 <= int(b) < MAX_BONES:
                raise ValueError('parts: bone %r outside [0, %d)' % (b, MAX_BONES))
            masks[int(b)] |= np.uint32(1 << p)
    return masks


def _check_radius(radius):
    if int(radius) != radius or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError('radius must be an integer in [1, %d], got %r' % (MAX_RADIUS, radius))
    return int(radius)


def twin_segment(rec, bone_masks, H, W, radius):
    """One frame's part membership in numpy, the bitmap statement of include/hnrf_segment.h: rec (N, 10),
    bone_masks (B,) uint32 -> member (N,) uint32, bit p set iff a record that seeds part p lies at L1 pixel distance
    < radius.  A row, column or bone that is not integer-valued, or a pixel outside [0, H) x [0, W): ValueError."""
    rec = np.asarray(rec, dtype=np.float32).reshape(-1, 10)
    masks = np.asarray(bone_masks).astype(np.uint32).reshape(-1)
    H, W, radius = int(H), int(W), _check_radius(radius)
    pix, bone = rec[:, 7:9], rec[:, 9]
    whole = lambda v: np.isfinite(v) & (v == np.floor(v)) & (np.abs(v) <= 2.0 ** 24)
    if not whole(pix).all():
        raise ValueError('twin_segment: a row or column that is not integer-valued')
    r, c = pix[:, 0].astype(np.int64), pix[:, 1].astype(np.int64)
    if ((r < 0) | (r >= H) | (c < 0) | (c >= W)).any():
        raise ValueError('twin_segment: a pixel outside the %d x %d image' % (H, W))
    if not whole(bone).all():
        raise ValueError('twin_segment: a bone index that is not integer-valued')
    b = bone.astype(np.int64)
    seeds = np.where((b >= 0) & (b < masks.size), masks[np.clip(b, 0, masks.size - 1)], np.uint32(0))
    seed = np.zeros((H + 2 * radius, W + 2 * radius), np.uint32)         # the image with a margin that seeds nothing
    np.bitwise_or.at(seed, (r + radius, c + radius), seeds)
    member = np.zeros(rec.shape[0], np.uint32)
    for dr in range(1 - radius, radius):
        w = radius - 1 - abs(dr)
        for dc in range(-w, w + 1):
            member |= seed[r + radius + dr, c + radius + dc]
    return member


def twin_compact(members, n_parts, weights=None, weight_min=0.0):
    """hnrf_segment_count / _scatter in numpy: ``members`` = the per-frame member words -> (seg_offsets (P F + 1,) int64,
    src (rows,) int32): per (part, frame), part-major, the packed rows whose bit is set (and, with ``weights`` = the
    per-frame columns 6, whose weight is > weight_min), ascending."""
    F = len(members)
    starts = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
    seg, src = [0], []
    for p in range(int(n_parts)):
        for f in range(F):
            keep = ((np.asarray(members[f]).astype(np.uint32) >> np.uint32(p)) & np.uint32(1)).astype(bool)
            if weights is not None:
                keep &= np.asarray(weights[f], dtype=np.float32) > np.float32(weight_min)
            rows = starts[f] + np.nonzero(keep)[0]
            src.append(rows)
            seg.append(seg[-1] + rows.size)
    return np.asarray(seg, np.int64), (np.concatenate(src) if src else np.zeros(0)).astype(np.int32)


def _image_size(recs, image_size):
    """(H, W): as given, or max row + 1 and max column + 1 over all frames' records (1 x 1 without records)."""
    if image_size is not None:
        H, W = int(image_size[0]), int(image_size[1])
        if H < 1 or W < 1:
            raise ValueError('image_size must be positive, got %r' % (image_size,))
        return H, W
    hi = [np.asarray(_host(r), dtype=np.float32)[:, 7:9].max(axis=0) for r in recs if r is not None and len(r)]
    if not hi:
        return 1, 1
    top = np.max(hi, axis=0)
    if not np.isfinite(top).all():
        raise ValueError('a row or column that is not finite')
    return int(top[0]) + 1, int(top[1]) + 1


def _segment_pack(recs, dev):
    """Device records -> the packed batch of include/hnrf_segment.h: rec (total, 10) and offsets (F + 1,) int64."""
    import torch
    counts = [r.shape[0] for r in recs]
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), device=dev)
    rec = torch.cat(recs).contiguous() if recs else torch.zeros(0, 10, device=dev)
    return rec, offsets


def _to_dev(rec, dev):
    import torch
    rec = torch.as_tensor(rec).to(dev, torch.float32)
    if rec.dim() != 2 or rec.shape[1] != 10:
        raise ValueError('a record must be [N, 10], got %s' % (tuple(rec.shape),))
    return rec


def segment_records(records, parts=None, radius=10, image_size=None, backend='hip', device=None):
    """tools/segment.py:23-49: ``records`` maps frame name -> [N, 10] record tensor (or None) -> {part: {frame name:
    tensor [n, 10] or None}}, the records within L1 pixel distance < ``radius`` of a record whose bone seeds the part,
    in record order; None where there is none (and for a None record).  ``parts``: name -> bones, default BODY_PARTS;
    ``image_size`` (H, W): None = max row + 1, max column + 1 over all frames.  Every record of a frame takes part (the
    weight filter belongs to the distance step).  'hip': one membership + compaction over all frames
    (hnrf_segment_members / _count / _scatter) and one gather per part; the results are CPU tensors.  'twin':
    twin_segment per frame."""
    import torch
    if backend not in ('hip', 'twin'):
        raise ValueError("backend must be 'hip' or 'twin'")
    parts = BODY_PARTS if parts is None else parts
    masks, radius = bone_masks(parts), _check_radius(radius)
    names = [n for n in records if records[n] is not None]
    H, W = _image_size([records[n] for n in names], image_size)
    out = {p: {n: None for n in records} for p in parts}
    if backend == 'twin':
        for n in names:
            rec = torch.as_tensor(records[n]).detach().cpu().to(torch.float32)
            member = twin_segment(rec.numpy(), masks, H, W, radius)
            for p, part in enumerate(parts):
                rows = np.nonzero((member >> np.uint32(p)) & np.uint32(1))[0]
                if rows.size:
                    out[part][n] = rec[torch.from_numpy(rows)]
        return out
    from . import ops
    dev = _device(device)
    rec, offsets = _segment_pack([_to_dev(records[n], dev) for n in names], dev)
    member, status = ops.segment_members(rec, offsets, torch.from_numpy(masks.view(np.int32)).to(dev), H, W, radius)
    seg, src = ops.segment_compact(member, offsets, len(parts), status=status)
    seg, F = seg.tolist(), len(names)
    for p, part in enumerate(parts):
        rows = rec[src[seg[p * F]:seg[(p + 1) * F]].long()].cpu()       # the part's records of all frames: one gather
        for f, n in enumerate(names):
            a, b = seg[p * F + f] - seg[p * F], seg[p * F + f + 1] - seg[p * F]
            if b > a:
                out[part][n] = rows[a:b]
    return out


def segment_distance_matrices(records, parts=None, radius=10, image_size=None, valid_weight_threshold=0.3,
                              dist_thresh=0.002, chunk=(0, 1), axis=None, backend='hip', device=None,
                              pairs_per_launch=1 << 16):
    """tools/compute_distance_seg.py over every part at once: {part: np.float32 [F, F]}, what distance_matrix gives on
    segment_records(...)[part], from ONE pack.  Every frame (sorted name order) is sorted once along ``axis`` with a
    stable sort, membership runs on the sorted rows, and the compaction keeps per (part, frame) the members with column
    6 > ``valid_weight_threshold`` -- a stable compaction of a sorted frame is sorted, so the P F segments are the clouds
    of hnrf_cloud_distance_pairs as they stand, with ``orig`` = the record's index in its frame (a monotone relabelling
    of its index inside the filtered segment: ties fall the same way).  ``axis``: None = the axis of largest extent over
    the points that pass the weight filter."""
    if backend not in ('hip', 'twin'):
        raise ValueError("backend must be 'hip' or 'twin'")
    tau = float(dist_thresh)
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError('dist_thresh must be finite and > 0, got %r' % dist_thresh)
    parts = BODY_PARTS if parts is None else parts
    masks, radius, P = bone_masks(parts), _check_radius(radius), len(parts)
    names = sorted(records.keys())
    F = len(names)
    have = [records[n] is not None for n in names]
    H, W = _image_size([records[n] for n in names], image_size)
    rows = chunk_rows(F, chunk)
    todo = [(i, j) for i in dict.fromkeys(rows.tolist()) for j in range(i + 1, F) if have[i] and have[j]]
    out = {part: np.zeros((F, F), dtype=np.float32) for part in parts}
    vwt = float(valid_weight_threshold)
    if backend == 'twin':
        recs = [np.asarray(_host(records[n]), dtype=np.float32).reshape(-1, 10) if have[k] else np.zeros((0, 10), np.float32)
                for k, n in enumerate(names)]
        if axis is None:
            axis = default_axis([r[r[:, 6] > np.float32(vwt)][:, :3] for r in recs])
        axis = int(axis)
        order = [np.argsort(r[:, axis], kind='stable') for r in recs]
        recs = [r[o] for r, o in zip(recs, order)]
        members = [twin_segment(r, masks, H, W, radius) for r in recs]
        seg, src = twin_compact(members, P, weights=[r[:, 6] for r in recs], weight_min=vwt)
        cat, ocat = np.concatenate(recs), np.concatenate(order).astype(np.int32)
        cloud = lambda s: (lambda k: {'xyz': _f32(cat[k, 0:3]), 'rgb': _f32(cat[k, 3:6]), 'orig': ocat[k]})(
            src[seg[s]:seg[s + 1]])
        for p, part in enumerate(parts):
            frames = {k: cloud(p * F + k) for k in range(F) if have[k]}
            for i, j in todo:
                out[part][i, j] = out[part][j, i] = twin_pairs(frames[i], frames[j], tau, axis, 'window')[2]
        return out
    import torch
    from . import ops
    dev = _device(device)
    recs = [_to_dev(records[n], dev) if have[k] else torch.zeros(0, 10, device=dev) for k, n in enumerate(names)]
    if axis is None:
        kept = [r[r[:, 6] > vwt][:, :3] for r in recs]
        ext = [torch.stack([x.min(0)[0], x.max(0)[0]]) for x in kept if x.shape[0]]
        axis = 0 if not ext else int(torch.argmax(torch.stack([e[1] for e in ext]).max(0)[0]
                                                  - torch.stack([e[0] for e in ext]).min(0)[0]))
    axis = int(axis)
    order = [torch.sort(r[:, axis], stable=True)[1] for r in recs]
    rec, offsets = _segment_pack([r[o] for r, o in zip(recs, order)], dev)
    member, status = ops.segment_members(rec, offsets, torch.from_numpy(masks.view(np.int32)).to(dev), H, W, radius)
    seg, src = ops.segment_compact(member, offsets, P, status=status, weight_rec=rec, weight_min=vwt)
    if not todo or src.numel() == 0:
        return out
    rows = rec[src.long()]
    xyz, rgb = rows[:, 0:3].contiguous(), rows[:, 3:6].contiguous()
    orig = (torch.cat(order).to(torch.int32))[src.long()].contiguous()
    max_n = int((seg[1:] - seg[:-1]).max())
    seg_dev = seg.to(dev)
    pairs_all = np.asarray([(p * F + i, p * F + j) for p in range(P) for i, j in todo], dtype=np.int32)
    vals = np.empty(pairs_all.shape[0], dtype=np.float64)
    for s in range(0, pairs_all.shape[0], int(pairs_per_launch)):
        pairs = torch.from_numpy(pairs_all[s:s + int(pairs_per_launch)]).to(dev)
        d, _ = ops.cloud_distance_pairs(xyz, rgb, orig, seg_dev, pairs, tau, axis, max_n)
        vals[s:s + pairs.shape[0]] = d.cpu().numpy()
    ti, tj = np.asarray(todo).T
    for p, part in enumerate(parts):
        v = vals[p * len(todo):(p + 1) * len(todo)]
        out[part][ti, tj] = v
        out[part][tj, ti] = v
    return out


def cluster_frames(D, n_clusters=4, names=None):
    """tools/cluster.py:21-50 in numpy: ``n_clusters`` groups of M = N // n_clusters frames grown greedily from the
    distance matrix D [N, N].  Per cluster: the seed is the lowest index not yet clustered; d = D[seed] with +inf at
    the seed and at everything clustered; then M - 1 times i = the first argmin of d joins, d[i] is recorded and
    d = max(D[i], d) with +inf at the cluster's members.  Returns the reference's list of {'names', 'dist'} (``names``:
    None = the indices); the N % n_clusters frames left over stay unclustered.  A matrix that is not finite,
    n_clusters < 1 or N < n_clusters: ValueError (the reference's argmin would pick a NaN, its seed search would raise).
    On the host by design: N^2 comparisons in N dependent steps."""
    D = np.asarray(D)
    if D.ndim != 2 or D.shape[0] != D.shape[1]:
        raise ValueError('D must be [N, N], got %s' % (D.shape,))
    if not np.issubdtype(D.dtype, np.floating):
        D = D.astype(np.float64)
    N, n_clusters = D.shape[0], int(n_clusters)
    if n_clusters < 1 or N < n_clusters:
        raise ValueError('n_clusters must be in [1, N = %d], got %d' % (N, n_clusters))
    if not np.isfinite(D).all():
        raise ValueError('D must be finite')
    names = list(range(N)) if names is None else list(names)
    if len(names) != N:
        raise ValueError('%d names for %d frames' % (len(names), N))
    M, inf = N // n_clusters, D.dtype.type(np.inf)
    clustered, results = np.zeros(N, bool), []
    for _ in range(n_clusters):
        seed = int(np.argmin(clustered))                                 # the first False
        members, dist = [seed], []
        d = D[seed].copy()
        d[clustered] = inf
        d[seed] = inf
        for _ in range(M - 1):
            i = int(np.argmin(d))
            members.append(i)
            dist.append(float(d[i]))
            d = np.maximum(D[i], d)
            d[members] = inf
        clustered[members] = True
        results.append({'names': [names[s] for s in members], 'dist': dist})
    return results


def merge_matrix_chunks(paths):
    """tools/merge_d.py: the sum of the chunk matrices (every chunk fills its own rows and their mirror, zeros
    elsewhere).  ``paths``: files or arrays; at least one.  The sum is the tool's: where the tail rows that chunk_rows
    gives the last chunk hold a pair of their own (F mod chunk_n >= 2), another chunk owns that pair too and it is
    counted twice, as in the reference."""
    mats = [np.load(p) if isinstance(p, (str, bytes)) or hasattr(p, '__fspath__') else np.asarray(p) for p in paths]
    if not mats:
        raise ValueError('merge_matrix_chunks: no chunk')
    if any(m.shape != mats[0].shape for m in mats):
        raise ValueError('merge_matrix_chunks: shapes differ: %s' % ([m.shape for m in mats],))
    return sum(mats[1:], mats[0].copy())
