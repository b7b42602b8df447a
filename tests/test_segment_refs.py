"""Body-part segmentation and frame clustering without a GPU (include/hnrf_segment.h, humannerf_amd/cloud.py): the numpy
twin against the reference's own loops (tests/golden/segments.npz, written by tests/make_golden_segments.py from
tools/segment.py and tools/cluster.py), its edges, the drivers' files and the argument checks of the C entries.
Everything here is integer arithmetic and selection: every comparison is exact."""
import os
import pickle

import numpy as np
import pytest
import torch

from humannerf_amd import cloud, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXIS, TAU = 1, 0.03


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'segments.npz'))


@pytest.fixture(scope='module')
def golden_records(golden):
    return {str(n): torch.from_numpy(golden['seg/rec/%s' % n]) for n in golden['seg/frames']}


def record(pixels, bones, weight=0.9):
    """[n, 10] with distinct coordinates: xyz by the record's index, weight, the given pixels and bones."""
    pixels = np.asarray(pixels, dtype=np.float32).reshape(-1, 2)
    n = pixels.shape[0]
    k = np.arange(n, dtype=np.float32)[:, None]
    return np.concatenate([k * [0.01, 0.02, 0.03], k * [0.1, 0.2, 0.3] % 1.0, np.full((n, 1), weight), pixels,
                           np.asarray(bones, dtype=np.float32).reshape(n, 1)], axis=1).astype(np.float32)


def member_bits(rec, parts, H, W, radius=10):
    return cloud.twin_segment(rec, cloud.bone_masks(parts), H, W, radius)


def test_the_part_table_is_the_references(golden):
    assert list(cloud.BODY_PARTS) == [str(p) for p in golden['seg/parts']] and len(cloud.BODY_PARTS) == 15
    bones = sorted(b for ls in cloud.BODY_PARTS.values() for b in ls)
    assert bones == list(range(24))                                       # every bone of the skeleton in exactly one part
    masks = cloud.bone_masks()
    assert masks.dtype == np.uint32 and masks.shape == (32,) and masks[7] == masks[10] == 1 << 5 and not masks[24:].any()


def test_twin_reproduces_the_reference_segments(golden, golden_records):
    H, W = int(golden['seg/H']), int(golden['seg/W'])
    seg = cloud.segment_records(golden_records, image_size=(H, W), backend='twin')
    nones = 0
    for part in cloud.BODY_PARTS:
        assert list(seg[part]) == list(golden_records)
        for name, rec in golden_records.items():
            got = seg[part][name]
            if int(golden['seg/none/%s/%s' % (part, name)]):
                assert got is None
                nones += 1
            else:
                rows = golden['seg/rows/%s/%s' % (part, name)]
                assert rows.size and np.array_equal(got.numpy(), rec.numpy()[rows])      # the rows, in the tool's order
    assert nones >= 10
    # image_size None = max row + 1, max column + 1: the same selection (the clipping never decides)
    auto = cloud.segment_records(golden_records, backend='twin')
    for part in cloud.BODY_PARTS:
        for name in golden_records:
            a, b = auto[part][name], seg[part][name]
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    # the generator's own claims about the tiny frame: L1 = 9 inside, L1 = 10 outside
    tiny = 'f002_tiny'
    assert golden['seg/rows/head/' + tiny].tolist() == [0, 1] and golden['seg/rows/lhip/' + tiny].tolist() == [0, 1, 2]
    assert golden['seg/rows/rhip/' + tiny].tolist() == [1, 2]


@pytest.mark.parametrize('case', ['ints22', 'floats9', 'each_alone'])
def test_cluster_frames_reproduces_the_reference(golden, case):
    D, k = golden['cluster/%s/D' % case], int(golden['cluster/%s/n_clusters' % case])
    names = ['frame_%03d.png' % i for i in range(D.shape[0])]
    got = cloud.cluster_frames(D, n_clusters=k, names=names)
    members, dist = golden['cluster/%s/members' % case], golden['cluster/%s/dist' % case]
    assert len(got) == k and members.shape == (k, D.shape[0] // k)
    for c, m, d in zip(got, members, dist):
        assert c['names'] == [names[i] for i in m] and c['dist'] == d.tolist()
        assert all(type(v) is float for v in c['dist'])
    assert [c['names'] for c in cloud.cluster_frames(D, n_clusters=k)] == members.tolist()
    if case == 'floats9':
        assert sorted(i for m in members for i in m) != list(range(9))    # one frame is left over, as in the reference


def test_cluster_frames_refuses_what_the_reference_cannot_run():
    D = np.ones((4, 4), np.float32)
    for bad in (np.nan, np.inf):
        E = D.copy()
        E[1, 2] = bad
        with pytest.raises(ValueError):
            cloud.cluster_frames(E, 2)
    for k in (0, -1, 5):
        with pytest.raises(ValueError):
            cloud.cluster_frames(D, k)
    with pytest.raises(ValueError):
        cloud.cluster_frames(D[:3], 2)
    with pytest.raises(ValueError):
        cloud.cluster_frames(D, 2, names=['a'])
    # an integer matrix is clustered as floats; ties go to the first minimum
    got = cloud.cluster_frames(np.zeros((4, 4), np.int64), 2)
    assert got == [{'names': [0, 1], 'dist': [0.0]}, {'names': [2, 3], 'dist': [0.0]}]


@pytest.mark.parametrize('radius', [1, 10, 33])
def test_the_boundary_is_l1_less_than_radius(radius):
    parts = {'a': [3]}
    for dr in range(0, radius, max(1, radius // 3)):
        inside, outside = (40 + dr, 40 + radius - 1 - dr), (40 + dr, 40 + radius - dr)
        m = member_bits(record([(40, 40), inside, outside, (40 - dr, 40 - (radius - dr))], [3, 0, 0, 0]), parts, 90, 90, radius)
        assert m.tolist() == [1, 1, 0, 0], (radius, dr)


def test_images_narrower_than_the_diamond_corners_and_shared_pixels():
    # 7 x 300: every diamond leaves the image above and below
    rs = np.random.RandomState(3)
    pix = np.stack([rs.randint(0, 7, 400), rs.randint(0, 300, 400)], 1)
    rec = record(pix, rs.randint(0, 24, 400))
    m = member_bits(rec, None, 7, 300)
    l1 = np.abs(pix[:, None, :] - pix[None, :, :]).sum(-1)
    for p, bones in enumerate(cloud.BODY_PARTS.values()):
        seeds = np.isin(rec[:, 9], bones)
        want = (l1[:, seeds].min(axis=1) < 10) if seeds.any() else np.zeros(400, bool)
        assert np.array_equal((m >> np.uint32(p)) & 1, want.astype(np.uint32))
    # seeds in all four corners; two records on one pixel seed different parts
    rec = record([(0, 0), (6, 299), (0, 299), (6, 0), (3, 150), (3, 150), (3, 141), (3, 140)], [0, 15, 3, 0, 15, 3, 23, 23])
    m = member_bits(rec, {'root': [0], 'head': [15], 'belly': [3]}, 7, 300)
    assert m.tolist() == [1, 6, 6, 1, 6, 6, 6, 0]


def test_custom_parts_overlap_and_reach_bit_31():
    parts = {'p%02d' % p: [p % 24] for p in range(32)}                    # bones 0 .. 7 seed two parts each
    parts['p31'] = [23, 5]
    masks = cloud.bone_masks(parts)
    assert masks[0] == (1 | 1 << 24) and masks[23] == (1 << 23 | 1 << 31) and masks[5] == (1 << 5 | 1 << 29 | 1 << 31)
    rec = record([(5, 5), (5, 9), (30, 30)], [23, 0, 5])
    m = cloud.twin_segment(rec, masks, 40, 56, 10)
    assert m.dtype == np.uint32
    assert m.tolist() == [1 << 23 | 1 << 31 | 1 | 1 << 24] * 2 + [1 << 5 | 1 << 29 | 1 << 31]
    seg = cloud.segment_records({'f': torch.from_numpy(rec)}, parts=parts, backend='twin')
    assert seg['p31']['f'].shape == (3, 10) and seg['p23']['f'].shape == (2, 10) and seg['p01']['f'] is None
    with pytest.raises(ValueError):
        cloud.bone_masks({'p%d' % p: [0] for p in range(33)})
    with pytest.raises(ValueError):
        cloud.bone_masks({})
    with pytest.raises(ValueError):
        cloud.bone_masks({'a': [32]})
    # a bone that is in no part, or outside the table, seeds nothing
    assert member_bits(record([(1, 1), (1, 2)], [7, 40]), {'a': [3]}, 4, 4).tolist() == [0, 0]


def test_empty_and_none_frames():
    recs = {'a': torch.zeros(0, 10), 'b': None, 'c': torch.from_numpy(record([(2, 3)], [15]))}
    seg = cloud.segment_records(recs, backend='twin')
    assert all(seg[p]['a'] is None and seg[p]['b'] is None for p in cloud.BODY_PARTS)
    assert torch.equal(seg['head']['c'], recs['c']) and seg['root']['c'] is None
    assert cloud.twin_segment(np.zeros((0, 10), np.float32), cloud.bone_masks(), 4, 4, 10).shape == (0,)
    seg_offsets, src = cloud.twin_compact([np.zeros(0, np.uint32), np.uint32([1, 2, 3])], 2)
    assert seg_offsets.tolist() == [0, 0, 2, 2, 4] and src.tolist() == [0, 2, 1, 2]
    D = cloud.segment_distance_matrices(recs, backend='twin', axis=0)
    assert sorted(D) == sorted(cloud.BODY_PARTS) and all(d.shape == (3, 3) and not d.any() for d in D.values())


@pytest.mark.parametrize('column, value', [(7, 2.5), (8, np.nan), (7, np.inf), (7, -1.0), (7, 40.0), (8, 56.0), (9, 1.5),
                                           (9, np.nan)])
def test_bad_records_are_refused_not_truncated(column, value):
    rec = record([(2, 3), (4, 5)], [15, 0])
    rec[1, column] = value
    with pytest.raises(ValueError):
        cloud.twin_segment(rec, cloud.bone_masks(), 40, 56, 10)
    with pytest.raises(ValueError):
        cloud.segment_records({'f': torch.from_numpy(rec)}, image_size=(40, 56), backend='twin')
    for radius in (0, 65, 2.5):
        with pytest.raises(ValueError):
            cloud.segment_records({'f': torch.from_numpy(record([(2, 3)], [15]))}, radius=radius, backend='twin')


def test_fused_matrices_equal_the_per_part_route(golden, golden_records, tmp_path):
    H, W = int(golden['seg/H']), int(golden['seg/W'])
    recs = dict(golden_records)
    rs = np.random.RandomState(5)
    for k in range(4):                                                    # more frames: jittered copies of the big one
        r = golden_records['f000_big'].numpy().copy()[rs.permutation(700)[:300 + 50 * k]]
        r[:, :3] += rs.uniform(-0.004, 0.004, r[:, :3].shape).astype(np.float32)
        assert np.unique(r[:, AXIS]).size == r.shape[0]
        recs['g%03d' % k] = torch.from_numpy(r)
    recs['h_none'] = None
    names = sorted(recs)
    F = len(names)
    seg = cloud.segment_records(recs, image_size=(H, W), backend='twin')
    full = cloud.segment_distance_matrices(recs, image_size=(H, W), dist_thresh=TAU, axis=AXIS, backend='twin')
    assert list(full) == list(cloud.BODY_PARTS)
    busy = 0
    for part in cloud.BODY_PARTS:
        want = cloud.distance_matrix(seg[part], dist_thresh=TAU, axis=AXIS, backend='twin')
        assert full[part].dtype == np.float32 and np.array_equal(full[part], want), part
        busy += bool(want.any())
    assert busy >= 6                                                      # (the comparison is not one of zeros)
    # the three chunk matrices add up to the full one (F = 8: chunk_rows' tail rows {6, 7} -- pair (6, 7) belongs to
    # chunk 0 as well, and the sum of tools/merge_d.py counts it twice: the reference's rule, kept)
    chunks = [cloud.segment_distance_matrices(recs, image_size=(H, W), dist_thresh=TAU, axis=AXIS, chunk=(c, 3),
                                              backend='twin') for c in range(3)]
    twice = np.zeros((F, F), np.float32)
    for i in cloud.chunk_rows(F, (2, 3)).tolist()[len(range(2, F, 3)):]:
        for j in range(i + 1, F):
            twice[i, j] = twice[j, i] = 1
    for part in ('head', 'belly', 'rwrist-hand'):
        merged = cloud.merge_matrix_chunks([c[part] for c in chunks])
        assert np.array_equal(merged, full[part] * (1 + twice))
    seven = {n: recs[n] for n in names[:7]}                               # F = 7: the tail row has no pair of its own
    full7 = cloud.segment_distance_matrices(seven, image_size=(H, W), dist_thresh=TAU, axis=AXIS, backend='twin')
    paths = []
    for c in range(3):
        res = run.run_segment_distance_matrices(seven, parts={'head': [15]}, image_size=(H, W), dist_thresh=TAU,
                                                axis=AXIS, chunk=(c, 3), backend='twin', out_dir=str(tmp_path))
        paths.append(res['paths']['head'])
        assert paths[-1] == str(tmp_path / 'distance_mat_seg' / 'head' / ('distance_mat_0.30-0.03.%d-3.npy' % c))
    assert full7['head'].any() and np.array_equal(cloud.merge_matrix_chunks(paths), full7['head'])
    with pytest.raises(ValueError):
        cloud.merge_matrix_chunks([])
    with pytest.raises(ValueError):
        cloud.segment_distance_matrices(recs, dist_thresh=0.0, backend='twin')


def test_drivers_write_the_references_tree(golden_records, tmp_path):
    path = str(tmp_path / 'name-2-3d.bin')
    torch.save(dict(golden_records, z_none=None), path)
    res = run.run_segments(path, backend='twin')
    assert sorted(res['paths']) == sorted(cloud.BODY_PARTS)
    for part, p in res['paths'].items():
        assert p == str(tmp_path / ('name-2-3d.%s.bin' % part))
        back = torch.load(p, map_location='cpu')
        assert list(back) == list(golden_records) + ['z_none'] and back['z_none'] is None
        for name, want in res['segments'][part].items():
            assert (back[name] is None) == (want is None) and (want is None or torch.equal(back[name], want))
    assert res['segments']['rhip']['f000_big'] is None and res['segments']['head']['f000_big'].shape[1] == 10
    # a part file is a records file: the whole-body driver reads it
    one = run.run_distance_matrix(res['paths']['head'], dist_thresh=TAU, axis=AXIS, backend='twin', out_dir=str(tmp_path / 'h'))
    mats = run.run_segment_distance_matrices(path, dist_thresh=TAU, axis=AXIS, backend='twin')
    assert mats['names'] == sorted(golden_records) + ['z_none']
    for part, p in mats['paths'].items():
        assert p == str(tmp_path / 'distance_mat_seg' / part / 'distance_mat_0.30-0.03.npy')
        assert np.array_equal(np.load(p), mats['matrices'][part])
    assert np.array_equal(mats['matrices']['head'], one['matrix']) and one['matrix'].any()
    # clusters: next to the matrix, .npy -> .cluster.pkl; from a path, from run_distance_matrix's result, from an array
    got = run.run_cluster(mats['paths']['head'], n_clusters=2)
    assert got['path'] == str(tmp_path / 'distance_mat_seg' / 'head' / 'distance_mat_0.30-0.03.cluster.pkl')
    with open(got['path'], 'rb') as f:
        assert pickle.load(f) == got['clusters'] == cloud.cluster_frames(mats['matrices']['head'], 2)
    named = run.run_cluster(one, n_clusters=2)
    assert named['path'] == one['path'][:-4] + '.cluster.pkl' and os.path.isfile(named['path'])
    assert named['clusters'][0]['names'][0] == 'f000_big' and len(named['clusters']) == 2
    assert [len(c['names']) for c in named['clusters']] == [2, 2] and [len(c['dist']) for c in named['clusters']] == [1, 1]
    loose = run.run_cluster(one['matrix'], names=one['names'], n_clusters=2)
    assert loose['path'] is None and loose['clusters'] == named['clusters']
    out = run.run_cluster(one['matrix'], n_clusters=4, out_path=str(tmp_path / 'c.pkl'))
    assert os.path.isfile(out['path']) and [c['names'] for c in out['clusters']] == [[0], [1], [2], [3]]


def test_segment_entries_are_additive_to_abi_13():
    from humannerf_amd import _lib
    assert sorted(_lib.SEGMENT_SIGNATURES) == ['hnrf_segment_compact_workspace_bytes', 'hnrf_segment_count',
                                               'hnrf_segment_members', 'hnrf_segment_scatter',
                                               'hnrf_segment_workspace_bytes']
    assert not set(_lib.SEGMENT_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.CLOUD_SIGNATURES) | set(_lib.VIDEO_SIGNATURES))
    lib = _lib.load_segment()
    assert lib.hnrf_abi_version() == 13
    up = lambda n: -(-n // 256) * 256
    assert lib.hnrf_segment_workspace_bytes(16, 512, 512) == 16 * 512 * 512 * 4
    assert lib.hnrf_segment_workspace_bytes(3, 7, 300) == up(3 * 7 * 300 * 4)
    assert lib.hnrf_segment_workspace_bytes(1, 0, 56) == 0 and lib.hnrf_segment_workspace_bytes(1 << 20, 512, 512) == 0
    assert lib.hnrf_segment_compact_workspace_bytes(1000, 15) == up((15 * 4 + 1) * 8) + up(15 * 4 * 4)
    assert lib.hnrf_segment_compact_workspace_bytes(1000, 33) == 0 and lib.hnrf_segment_compact_workspace_bytes(-1, 15) == 0
    # refused before any launch, each naming its argument (no GPU is touched: the argument checks come first)
    members = lambda radius, bones, H: lib.hnrf_segment_members(1, 1, 1, 4, 1, bones, H, 56, radius, 1, 1 << 20, 1, 1, None)
    for args, word in (((0, 24, 40), b'radius'), ((65, 24, 40), b'radius'), ((10, 33, 40), b'n_bones'),
                       ((10, 24, -40), b'H ')):
        assert members(*args) == -1 and word in lib.hnrf_last_error(), lib.hnrf_last_error()
    assert lib.hnrf_segment_count(1, None, 0.0, 1, 1, 4, 33, None, 1, 1 << 20, 1, None) == -1
    assert b'n_parts' in lib.hnrf_last_error()
    assert lib.hnrf_segment_scatter(1, None, 0.0, 4, 33, None, 1, 1 << 20, 1, 4, None) == -1
    assert b'n_parts' in lib.hnrf_last_error()
    assert lib.hnrf_segment_scatter(1, None, 0.0, -4, 15, None, 1, 1 << 20, 1, 4, None) == -1
    assert b'total' in lib.hnrf_last_error()
    assert lib.hnrf_segment_count(1, None, float('nan'), 1, 1, 4, 15, None, 1, 1 << 20, 1, None) == -1
    assert b'weight_min' in lib.hnrf_last_error()
