"""Writes tests/golden/segments.npz: the reference's own tools/segment.py and tools/cluster.py loops on small inputs.

    python tests/make_golden_segments.py <path to a checkout of the reference>

A script, not a test.  Both tools run a whole job on hard-coded paths when they are imported, so only their loops are
taken out with ``ast`` at generation time and run on CPU tensors: of ``segment.py`` the ``name2cluster`` and
``name2res`` assignments and the first two ``for`` statements (``res`` injected, ``tqdm`` stubbed), of ``cluster.py``
the ``clustered`` and ``results`` assignments and the ``for`` statement (``D``, ``N``, ``M``, ``N_cluster``, ``names``
and a silent ``print`` injected).  Only data is stored:

  seg/frames                     the frame names;  seg/H, seg/W the image size;  seg/parts the part names
  seg/rec/<frame>                the [N, 10] records
  seg/rows/<part>/<frame>        the indices of the kept records, in the order the tool returns them
  seg/none/<part>/<frame>        1 where the tool stored None
  cluster/<case>/D, n_clusters   the input;  cluster/<case>/members [n_clusters, M] the clusters' indices, .../dist
                                 [n_clusters, M - 1] the recorded distances (as the tool's Python floats)

The records' coordinates are distinct along every axis within a frame (asserted): a sort along one is unique."""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'segments.npz')
H, W = 40, 56
BAND_BONES = (15, 12, 16, 3, 0, 1, 4, 7)        # the bone of rows 5 b .. 5 b + 4: several parts never occur


def _loops(checkout, tool, assigned, n_for):
    path = os.path.join(checkout, 'tools', tool)
    with open(path) as f:
        tree = ast.parse(f.read())
    body, fors = [], 0
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id in assigned for t in node.targets):
            body.append(node)
        elif isinstance(node, ast.For) and fors < n_for:
            body.append(node)
            fors += 1
    assert fors == n_for and len(body) == len(assigned) + n_for, path
    return compile(ast.Module(body=body, type_ignores=[]), path, 'exec')


def reference_segments(checkout, res):
    ns = {'torch': torch, 'np': np, 'tqdm': lambda it: it, 'res': res}
    exec(_loops(checkout, 'segment.py', ('name2cluster', 'name2res'), 2), ns)
    return ns['name2cluster'], ns['name2res']


def reference_clusters(checkout, D, n_clusters):
    N = D.shape[0]
    ns = {'torch': torch, 'np': np, 'print': lambda *a, **k: None, 'D': torch.from_numpy(D), 'N': N,
          'M': N // n_clusters, 'N_cluster': n_clusters, 'names': list(range(N))}
    exec(_loops(checkout, 'cluster.py', ('clustered', 'results'), 1), ns)
    return ns['results']


def frame(rs, n, pixels=None, bones=None):
    """[n, 10]: xyz near the pixel (so that parts of different frames meet) | rgb | weight | row, col | bone by band."""
    if pixels is None:
        flat = rs.choice(H * W, size=n, replace=False)
        pixels = np.stack([flat // W, flat % W], 1)
    pixels = np.asarray(pixels, dtype=np.int64)
    if bones is None:
        bones = np.asarray(BAND_BONES)[pixels[:, 0] // 5]
    xyz = np.stack([pixels[:, 1] / W + rs.uniform(-0.01, 0.01, n), pixels[:, 0] / H + rs.uniform(-0.01, 0.01, n),
                    rs.uniform(0, 0.05, n)], 1)
    rec = np.concatenate([xyz, rs.uniform(0, 1, (n, 3)), rs.uniform(0.1, 1.0, (n, 1)), pixels,
                          np.asarray(bones).reshape(n, 1)], axis=1).astype(np.float32)
    for a in range(3):
        assert np.unique(rec[:, a]).size == n, 'coordinates along axis %d are not distinct' % a
    assert np.unique(rec, axis=0).shape[0] == n
    return rec


def segment_cases():
    rs = np.random.RandomState(11)
    big = frame(rs, 700)
    mid = frame(rs, 257)
    mid[1, 7:9] = mid[0, 7:9]                    # two records on one pixel, of different bones
    mid[0, 9], mid[1, 9] = 20, 5
    mid[2, 7:10] = (H - 1, W - 1, 23)            # a seed in an image corner
    # a head seed in the corner (0, 0); a record at L1 distance exactly 9 from it (inside) that seeds lhip, and one at
    # exactly 10 (outside) that seeds rhip: head = {0, 1}, lhip = {0, 1, 2}, rhip = {1, 2}
    tiny = frame(rs, 3, pixels=[(0, 0), (4, 5), (5, 5)], bones=[15, 1, 2])
    return {'f000_big': big, 'f001_mid': mid, 'f002_tiny': tiny}


def cluster_cases():
    rs = np.random.RandomState(12)
    a = rs.randint(0, 4, (22, 22))
    ints = np.triu(a, 1) + np.triu(a, 1).T       # symmetric, zero diagonal, ties and zeros off it
    b = rs.uniform(0.1, 5.0, (9, 9))
    floats = np.triu(b, 1) + np.triu(b, 1).T
    c = rs.uniform(0.1, 5.0, (4, 4))
    return {'ints22': (ints.astype(np.float32), 4), 'floats9': (floats.astype(np.float32), 2),
            'each_alone': ((c + c.T).astype(np.float32), 4)}


def main(checkout):
    store = {}
    frames = segment_cases()
    parts, result = reference_segments(checkout, {k: torch.from_numpy(v) for k, v in frames.items()})
    store['seg/frames'], store['seg/parts'] = np.asarray(list(frames)), np.asarray(list(parts))
    store['seg/H'], store['seg/W'] = np.int64(H), np.int64(W)
    for name, rec in frames.items():
        store['seg/rec/' + name] = rec
        index = {tuple(row.tolist()): i for i, row in enumerate(rec)}
        for part in parts:
            got = result[part][name]
            rows = np.zeros(0, np.int32) if got is None else np.asarray([index[tuple(r.tolist())] for r in got.numpy()],
                                                                        dtype=np.int32)
            store['seg/rows/%s/%s' % (part, name)] = rows
            store['seg/none/%s/%s' % (part, name)] = np.int64(got is None)
        print('%-10s N %4d  parts present %2d  kept %s' % (name, rec.shape[0],
              sum(result[p][name] is not None for p in parts), [store['seg/rows/%s/%s' % (p, name)].size for p in parts]))
    for case, (D, k) in cluster_cases().items():
        res = reference_clusters(checkout, D, k)
        store['cluster/%s/D' % case], store['cluster/%s/n_clusters' % case] = D, np.int64(k)
        store['cluster/%s/members' % case] = np.asarray([c['names'] for c in res], dtype=np.int64).reshape(k, -1)
        store['cluster/%s/dist' % case] = np.asarray([c['dist'] for c in res], dtype=np.float64).reshape(k, -1)
        print('%-10s N %2d clusters %d' % (case, D.shape[0], k), [c['names'] for c in res])
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), 'bytes')
    assert os.path.getsize(OUT) <= 500 * 1000


if __name__ == '__main__':
    main(sys.argv[1])
