"""Writes tests/golden/cloud_pairs.npz: the reference's own find_nearest_pair_gpu / compute_distance_gpu on small clouds.

    python tests/make_golden_cloud.py <path to a checkout of the reference>

A script, not a test.  ``tools/compute_distance_seg.py`` runs a whole job when it is imported, so only its two function
definitions are taken out of it with ``ast`` at generation time and evaluated on CPU tensors (fp32, as the tool runs
them).  Stored per case ``<name>/...``: the two [N, 10] records (``none0`` / ``none1`` = 1 for a None record), tau and the
weight threshold, the reference's pair_0 / pair_1 (indices into the filtered clouds) and distance, the same functions'
distance on the records cast to fp64 (``distance64``) and ``deviation`` = |distance - distance64|, the reference's own
fp32 error.  ``ran`` = 0 marks a case the reference cannot evaluate (its argmin refuses an empty cloud): no pair exists
there, the distance is 0 by definition.

The cases are drawn so that every point is DECIDED (tests/test_cloud_refs.py: in fp64 the two best candidates differ by
more than 1e-5 relative and the nearest distance is more than 1e-5 tau away from tau) -- the script refuses to write
anything else -- except for the tie lattice, whose arithmetic is exact."""
import ast
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden', 'cloud_pairs.npz')
BOX = np.array([0.9, 1.8, 0.3])
VWT = 0.3


def reference_functions(checkout):
    path = os.path.join(checkout, 'tools', 'compute_distance_seg.py')
    with open(path) as f:
        tree = ast.parse(f.read())
    want = ('find_nearest_pair_gpu', 'compute_distance_gpu')
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert sorted(n.name for n in body) == sorted(want), path
    ns = {'torch': torch, 'time': time.time, 'np': np, 'framename2info': {}}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, 'exec'), ns)
    return ns


def record(rs, xyz, weight_lo=0.31):
    """[N, 10]: xyz | rgb uniform | weight max in (weight_lo, 1) | row, col | lbs."""
    n = xyz.shape[0]
    return np.concatenate([xyz, rs.uniform(0, 1, (n, 3)), rs.uniform(weight_lo, 1.0, (n, 1)),
                           rs.randint(0, 512, (n, 2)), rs.randint(0, 24, (n, 1))], axis=1).astype(np.float32)


def undecided(x0, x1, tau):
    """Share of the points of both clouds that are not decided (fp64)."""
    a, b = x0.astype(np.float64), x1.astype(np.float64)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return 0.0
    d = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    bad = 0
    for m in (d, d.T):
        s = np.sort(m, axis=1)
        near_tau = np.abs(s[:, 0] - tau) <= 1e-5 * tau
        tie = (s[:, 1] - s[:, 0] <= 1e-5 * s[:, 1]) if m.shape[1] > 1 else np.zeros(m.shape[0], bool)
        bad += int((near_tau | tie).sum())
    return bad / (a.shape[0] + b.shape[0])


def cases():
    rs = np.random.RandomState(7)
    out = {}
    # a jittered, permuted copy: every point pairs with its original
    x = rs.uniform(0, 1, (800, 3)) * BOX
    y = (x + rs.uniform(-1, 1, (800, 3)) * 2e-4)[rs.permutation(800)]
    out['jitter'] = (record(rs, x), record(rs, y), 0.002)
    # a partial, noisier copy: pairs on both sides of tau, points without partner, some under the weight threshold
    x = rs.uniform(0, 1, (900, 3)) * BOX
    y = (x[:700] + rs.normal(0, 1, (700, 3)) * 1.2e-3)[rs.permutation(700)]
    out['partial'] = (record(rs, x, weight_lo=0.2), record(rs, y, weight_lo=0.2), 0.002)
    # independent clouds of unequal size over the box, three thresholds
    x, y = rs.uniform(0, 1, (1500, 3)) * BOX, rs.uniform(0, 1, (1100, 3)) * BOX
    r0, r1 = record(rs, x), record(rs, y)
    for tau in (0.002, 0.02, 0.05):
        out['indep_%g' % tau] = (r0, r1, tau)
    # an integer lattice against its cell centres: four exactly equal nearest neighbours everywhere
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), indexing='ij'), -1).reshape(-1, 2)
    x = np.concatenate([g, np.zeros((g.shape[0], 1))], 1).astype(np.float64)
    y = (x + [0.5, 0.5, 0.0])[rs.permutation(x.shape[0])]
    out['lattice'] = (record(rs, x), record(rs, y), 1.0)
    out['single'] = (record(rs, np.array([[0.1, 0.2, 0.05]])), record(rs, np.array([[0.1005, 0.2, 0.05]])), 0.002)
    out['single_far'] = (record(rs, np.array([[0.1, 0.2, 0.05]])), record(rs, np.array([[0.3, 0.2, 0.05]])), 0.002)
    emptied = record(rs, rs.uniform(0, 1, (40, 3)) * BOX)
    emptied[:, 6] = rs.uniform(0.0, 0.29, 40)
    out['emptied'] = (emptied, record(rs, rs.uniform(0, 1, (50, 3)) * BOX), 0.05)
    out['none'] = (None, record(rs, rs.uniform(0, 1, (50, 3)) * BOX), 0.05)
    return out


def main(checkout):
    ns = reference_functions(checkout)
    store = {}
    for name, (r0, r1, tau) in cases().items():
        def run(dtype):
            info = {k: (None if r is None else torch.from_numpy(r).to(dtype)) for k, r in (('a', r0), ('b', r1))}
            ns['framename2info'] = info
            d = ns['compute_distance_gpu']('a', 'b', dist_thresh=tau, valid_weight_threshold=VWT)
            if info['a'] is None or info['b'] is None:
                return d, np.zeros(0, np.int64), np.zeros(0, np.int64)
            x0, x1 = (info[k][info[k][:, 6] > VWT][:, :3] for k in ('a', 'b'))
            p0, p1, _ = ns['find_nearest_pair_gpu'](x0, x1)
            return float(d), p0.reshape(-1).numpy(), p1.reshape(-1).numpy()
        ran = 1
        try:
            d32, p0, p1 = run(torch.float32)
            d64 = run(torch.float64)[0]
        except (IndexError, RuntimeError) as e:                          # argmin over an empty cloud
            assert r0 is not None and r1 is not None and min((r0[:, 6] > VWT).sum(), (r1[:, 6] > VWT).sum()) == 0, e
            ran, d32, d64, p0, p1 = 0, 0.0, 0.0, np.zeros(0, np.int64), np.zeros(0, np.int64)
        if r0 is not None and r1 is not None and name != 'lattice':
            u = undecided(r0[r0[:, 6] > VWT][:, :3], r1[r1[:, 6] > VWT][:, :3], tau)
            assert u == 0, (name, u)
        empty = np.zeros((0, 10), np.float32)
        store.update({name + '/rec0': empty if r0 is None else r0, name + '/rec1': empty if r1 is None else r1,
                      name + '/none0': np.int64(r0 is None), name + '/none1': np.int64(r1 is None),
                      name + '/tau': np.float64(tau), name + '/vwt': np.float64(VWT), name + '/ran': np.int64(ran),
                      name + '/pair_0': p0.astype(np.int32), name + '/pair_1': p1.astype(np.int32),
                      name + '/distance': np.float32(d32), name + '/distance64': np.float64(d64),
                      name + '/deviation': np.float64(abs(float(np.float32(d32)) - float(d64)))})
        print('%-12s N %4d %4d  tau %-6g pairs %4d  distance %.7g  deviation %.3g' % (
            name, 0 if r0 is None else r0.shape[0], 0 if r1 is None else r1.shape[0], tau, p0.size, d32,
            store[name + '/deviation']))
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), 'bytes')
    assert os.path.getsize(OUT) <= 500 * 1000


if __name__ == '__main__':
    main(sys.argv[1])
