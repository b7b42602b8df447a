"""Surface-point records and the frame x frame appearance distance: the reference's ``cfg.test.save_3d_together``
dump (run.py:388-404, image_util.py:99-119) and ``tools/compute_distance*.py`` on this package's kernels
(include/hnrf_cloud.h, csrc/hnrf_cloud.hip).

  surface_records   one record per ray whose largest weight passes the threshold: [N, 10] fp32 on the device, the
                    reference's columns -- weighted xyz (3) | image rgb (3) | weight max | pixel row, col | lbs argmax
  nearest_pairs     find_nearest_pair_gpu: the mutual nearest neighbours of two clouds
  frame_distance    compute_distance_gpu: the summed colour error of the mutual pairs closer than dist_thresh
  distance_matrix   the frame x frame matrix of the tools' main loop, all pairs of a chunk in one launch

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
