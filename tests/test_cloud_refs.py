"""Surface-point records and the frame distance without a GPU (include/hnrf_cloud.h, humannerf_amd/cloud.py): the numpy
twin of the kernels' arithmetic against the reference's own find_nearest_pair_gpu / compute_distance_gpu
(tests/golden/cloud_pairs.npz, written by tests/make_golden_cloud.py), the windowed search against the brute-force one,
the records against the torch expressions of run.py:391-404, the writer and the matrix driver.

torch.linalg.norm is not bit-equal to the twin's fl(sqrt(d2)), so parity with the reference is stated on decisions: a
point is DECIDED when, in fp64, its two best candidates differ by more than 1e-5 relative and its nearest distance is
more than 1e-5 tau away from tau.  The fixtures hold no undecided point (the tie lattice aside, whose arithmetic is
exact in every format), so there the pair sets must be equal outright."""
import os

import numpy as np
import pytest
import torch

from humannerf_amd import cloud, render, run
from humannerf_amd._lib import HnrfError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['jitter', 'partial', 'indep_0.002', 'indep_0.02', 'indep_0.05', 'lattice', 'single', 'single_far', 'emptied',
         'none']


@pytest.fixture(scope='module')
def golden():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'cloud_pairs.npz'))

    def get(name):
        c = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
        c['rec0'] = None if int(c['none0']) else c['rec0']
        c['rec1'] = None if int(c['none1']) else c['rec1']
        c['tau'], c['vwt'] = float(c['tau']), float(c['vwt'])
        return c
    assert sorted({k.split('/')[0] for k in z.files}) == sorted(CASES)
    return get


def _clouds(c):
    return [r[r[:, 6] > c['vwt']] for r in (c['rec0'], c['rec1'])]


def _undecided(x0, x1, tau):
    a, b = x0.astype(np.float64), x1.astype(np.float64)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return 0.0
    d = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    bad = 0
    for m in (d, d.T):
        s = np.sort(m, axis=1)
        tie = (s[:, 1] - s[:, 0] <= 1e-5 * s[:, 1]) if m.shape[1] > 1 else np.zeros(m.shape[0], bool)
        bad += int((tie | (np.abs(s[:, 0] - tau) <= 1e-5 * tau)).sum())
    return bad / (a.shape[0] + b.shape[0])


@pytest.mark.parametrize('name', CASES)
def test_twin_against_reference(golden, name):
    c = golden(name)
    if c['rec0'] is None or c['rec1'] is None:
        for method in ('window', 'brute'):
            d = cloud.frame_distance(c['rec0'], c['rec1'], c['vwt'], c['tau'], method=method, backend='twin')
            assert d == 0 and isinstance(d, int)
        return
    f0, f1 = _clouds(c)
    x0, x1 = f0[:, :3], f1[:, :3]
    if name != 'lattice':
        assert _undecided(x0, x1, c['tau']) == 0
    # the mutual pairs of find_nearest_pair_gpu
    p0, p1, d01, _ = cloud.twin_nearest_pairs(x0, x1)
    assert np.array_equal(p0, c['pair_0']) and np.array_equal(p1, c['pair_1'])
    # ... and those closer than tau, by the windowed search along every axis
    d64 = np.sqrt(((x0[p0].astype(np.float64) - x1[p1].astype(np.float64)) ** 2).sum(-1)) if p0.size else np.zeros(0)
    want = {(int(a), int(b)) for a, b, d in zip(p0, p1, d64) if d < c['tau']}
    for axis in range(3):
        s0, s1 = cloud.sort_frame(x0, f0[:, 3:6], axis), cloud.sort_frame(x1, f1[:, 3:6], axis)
        match = cloud.twin_pairs(s0, s1, c['tau'], axis)[0]
        assert {(int(o), int(m)) for o, m in zip(s0['orig'], match) if m >= 0} == want
    tol = max(4 * float(c['deviation']), 1e-6 * abs(float(c['distance64'])))
    for method in ('window', 'brute'):
        d = cloud.frame_distance(c['rec0'], c['rec1'], c['vwt'], c['tau'], method=method, backend='twin')
        print(name, method, d, float(c['distance64']), 'tol', tol)
        assert abs(d - float(c['distance64'])) <= tol
    if int(c['ran']):
        assert abs(float(c['distance']) - float(c['distance64'])) <= float(c['deviation']) * (1 + 1e-12)


SIZES = [(0, 5), (5, 0), (1, 1), (1, 257), (63, 64), (64, 65), (65, 63), (257, 64), (257, 257)]


def _random_cloud(rs, n):
    """Points in a 0.09 x 0.18 x 0.03 box, a third of them snapped to a 1/256 lattice (exact ties and duplicates)."""
    x = rs.uniform(0, 1, (n, 3)) * [0.09, 0.18, 0.03]
    snap = rs.rand(n) < 1 / 3
    x[snap] = np.round(x[snap] * 256) / 256
    return x.astype(np.float32)


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_window_equals_brute(axis):
    rs = np.random.RandomState(11 + axis)
    pairs_seen = 0
    for na, nb in SIZES:
        a, b = _random_cloud(rs, na), _random_cloud(rs, nb)
        fa = cloud.sort_frame(a, rs.rand(na, 3), axis)
        fb = cloud.sort_frame(b, rs.rand(nb, 3), axis)
        for tau in (1e-3, 4e-3, 0.02, 0.5):                              # ... 0.5: larger than the box
            mw, ew, dw = cloud.twin_pairs(fa, fb, tau, axis, 'window')
            mb, eb, db = cloud.twin_pairs(fa, fb, tau, axis, 'brute')
            assert np.array_equal(mw, mb) and np.array_equal(ew, eb) and dw == db, (na, nb, tau)
            pairs_seen += int((mw >= 0).sum())
            # per point: wherever the brute-force neighbour is closer than tau the window finds the same one
            qb, d2b = cloud.twin_nn(fa['xyz'], fb['xyz'], fb['orig'])
            qw, d2w = cloud.twin_window_nn(fa['xyz'], fb['xyz'], fb['orig'], axis, tau)
            near = (qb >= 0) & (np.sqrt(d2b) < np.float32(tau))
            assert np.array_equal(qw[near], qb[near]) and np.array_equal(d2w[near], d2b[near])
            assert not np.any((qw >= 0) & ~near & (np.sqrt(d2w) < np.float32(tau)))
    assert pairs_seen > 200


def test_twin_nn_lowest_index_is_torch_argmin():
    rs = np.random.RandomState(3)
    a = rs.randint(0, 4, (200, 3)).astype(np.float32)
    b = rs.randint(0, 4, (150, 3)).astype(np.float32)
    pos, d2 = cloud.twin_nn(a, b)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    dist = ((ta[:, None] - tb[None]) ** 2).sum(-1)
    assert np.array_equal(pos, torch.argmin(dist, dim=1).numpy())
    assert np.array_equal(d2, dist.min(dim=1)[0].numpy())


def _synthetic_outputs(R, S, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.softmax(10 * torch.randn(R, S, generator=g), -1) * torch.rand(R, 1, generator=g)      # one peak per ray
    return {'weights_on_rays': w, 'xyz_on_rays': torch.randn(R, S, 3, generator=g),
            'backward_motion_weights': torch.softmax(8 * torch.randn(R, S, B, generator=g), -1)}


def test_surface_records_against_torch_restatement():
    R, S, B, W = 97, 128, 24, 16
    out = _synthetic_outputs(R, S, B)
    g = torch.Generator().manual_seed(5)
    truth = torch.rand(R, 3, generator=g)
    ray_index = torch.sort(torch.randperm(20 * W, generator=g)[:R])[0]
    thr = 0.3
    rec = cloud.surface_records(out, truth, ray_index, W, thr, backend='twin')
    # run.py:391-404 (pos_on_image = the (row, col) of the pixels the rays go through)
    w, xyz, bmw = (out[k].double() for k in cloud.RECORD_KEYS)
    weighted_xyz = torch.sum(w[..., None] * xyz, axis=1)
    weight_max = torch.max(out['weights_on_rays'], axis=-1)[0][..., None]
    lbs = torch.sum(w[..., None] * bmw, axis=1)
    lbs_argmax = torch.argmax(lbs, axis=1)[..., None]
    mask = torch.zeros(20 * W, dtype=torch.bool)
    mask[ray_index] = True
    pos_on_image = mask.view(20, W).nonzero()
    save_mask = torch.max(out['weights_on_rays'], axis=1)[0] > thr
    want = torch.cat([weighted_xyz[save_mask], truth[save_mask].double(), weight_max[save_mask].double(),
                      pos_on_image[save_mask].double(), lbs_argmax[save_mask].double()], axis=1)
    assert 0 < int(save_mask.sum()) < R
    assert rec.dtype == torch.float32 and rec.shape == want.shape
    assert torch.equal(rec[:, 3:10].double(), want[:, 3:10])
    ref32 = torch.sum(out['weights_on_rays'][..., None] * out['xyz_on_rays'], axis=1)[save_mask].double()
    bound = 4 * float((ref32 - want[:, :3]).abs().max())
    assert float((rec[:, :3].double() - want[:, :3]).abs().max()) <= bound
    top2 = torch.topk(lbs, 2, dim=1)[0]
    assert bool(((top2[:, 0] - top2[:, 1]) > 1e-5 * top2[:, 0]).all())     # (the argmax above is decided)
    with pytest.raises(HnrfError, match='diagnostics'):
        cloud.surface_records({'weights_on_rays': out['weights_on_rays']}, truth, ray_index, W, thr, backend='twin')


def test_writer_round_trips_records(tmp_path):
    w = render.ImageWriter(str(tmp_path / 'a'), 'movement', workers=1)
    assert w.finalize() is None and not os.path.exists(str(tmp_path / 'a' / 'name-2-3d.bin'))
    w = render.ImageWriter(str(tmp_path / 'b'), 'movement', workers=1)
    recs = {'frame_000003': torch.rand(7, 10), 'cam/frame_000010': torch.rand(0, 10)}
    for k, v in recs.items():
        w.append_3d_together(k, v)
    w.finalize()
    got = torch.load(str(tmp_path / 'b' / 'name-2-3d.bin'))
    assert sorted(got) == sorted(recs)
    for k in recs:
        assert got[k].device.type == 'cpu' and torch.equal(got[k], recs[k])


def _records(rs, F, n=40):
    base = rs.uniform(0, 1, (n, 3)) * [0.09, 0.18, 0.03]
    recs = {}
    for k in range(F):
        m = n - (k % 3)
        xyz = base[:m] + rs.normal(0, 1, (m, 3)) * 1e-3
        recs['f%02d' % (F - k)] = torch.from_numpy(np.concatenate(       # (names not in insertion order)
            [xyz, rs.rand(m, 3), rs.uniform(0.2, 1.0, (m, 1)), rs.randint(0, 64, (m, 2)), rs.randint(0, 24, (m, 1))],
            1).astype(np.float32))
    return recs


def test_distance_matrix_chunks_symmetry_and_file(tmp_path):
    rs = np.random.RandomState(2)
    F = 7
    recs = _records(rs, F)
    recs['f03'] = None
    names = sorted(recs)
    full = cloud.distance_matrix(recs, dist_thresh=0.004, backend='twin')
    assert full.dtype == np.float32 and full.shape == (F, F)
    assert np.array_equal(full, full.T) and not full.diagonal().any()
    k = names.index('f03')
    assert not full[k].any() and np.count_nonzero(full) == (F - 1) * (F - 2)
    for i in range(F):
        for j in range(i + 1, F):
            want = cloud.frame_distance(recs[names[i]], recs[names[j]], dist_thresh=0.004, backend='twin', axis=1)
            assert full[i, j] == np.float32(want)
    assert np.array_equal(full, cloud.distance_matrix(recs, dist_thresh=0.004, backend='twin', method='brute', axis=2))
    # the chunk rule: rows arange(id, F, n), the last chunk also every row after its last one
    assert cloud.chunk_rows(7, (0, 3)).tolist() == [0, 3, 6]
    assert cloud.chunk_rows(7, (1, 3)).tolist() == [1, 4]
    assert cloud.chunk_rows(7, (2, 3)).tolist() == [2, 5, 6]
    assert cloud.chunk_rows(2, (2, 3)).tolist() == []
    total = np.zeros_like(full)
    for cid in range(3):
        part = cloud.distance_matrix(recs, dist_thresh=0.004, chunk=(cid, 3), backend='twin')
        rows = cloud.chunk_rows(F, (cid, 3))
        keep = np.zeros((F, F), bool)
        for i in rows:
            keep[i, i + 1:] = True
        keep |= keep.T
        assert np.array_equal(part, np.where(keep, full, 0))
        total = np.maximum(total, part)
    assert np.array_equal(total, full)
    with pytest.raises(ValueError):
        cloud.distance_matrix(recs, dist_thresh=float('nan'), backend='twin')
    with pytest.raises(ValueError):
        cloud.chunk_rows(7, (3, 3))
    # the driver and the reference's file names
    path = str(tmp_path / 'name-2-3d.bin')
    torch.save(recs, path)
    res = run.run_distance_matrix(path, dist_thresh=0.004, backend='twin')
    assert res['path'] == str(tmp_path / 'distance_mat' / 'distance_mat_0.30-0.00.npy') and res['names'] == names
    assert np.array_equal(np.load(res['path']), full)
    res = run.run_distance_matrix(recs, valid_weight_threshold=0.25, dist_thresh=0.02, chunk=(2, 3), backend='twin',
                                  out_dir=str(tmp_path / 'o'))
    assert res['path'] == str(tmp_path / 'o' / 'distance_mat' / 'distance_mat_0.25-0.02.2-3.npy')
    assert os.path.isfile(res['path'])


def test_cloud_entries_are_additive_to_abi_13():
    from humannerf_amd import _lib
    assert sorted(_lib.CLOUD_SIGNATURES) == ['hnrf_cloud_distance_pairs', 'hnrf_cloud_distance_pairs_workspace_bytes',
                                             'hnrf_cloud_nn', 'hnrf_surface_points']
    assert not set(_lib.CLOUD_SIGNATURES) & set(_lib.SIGNATURES)
    lib = _lib.load_cloud()
    assert lib.hnrf_abi_version() == 13
    up = lambda n: -(-n // 256) * 256
    assert lib.hnrf_cloud_distance_pairs_workspace_bytes(10, 700) == up(10 * 3 * 8)
    assert lib.hnrf_cloud_distance_pairs_workspace_bytes(1 << 20, 700) == up(65535 * 3 * 8)   # one launch's partials
    assert lib.hnrf_cloud_distance_pairs_workspace_bytes(-1, 700) == 0
    # refused before any launch (no GPU is touched: the argument checks come first)
    assert lib.hnrf_cloud_distance_pairs(None, None, None, None, 0, 0, None, 1, 0, 0, float('nan'), None, 0, None, None,
                                         None) == -1
    assert b'tau' in lib.hnrf_last_error()
    assert lib.hnrf_surface_points(1, 1, 1, 4, 513, 24, 1, 1, 1, None) == -2
