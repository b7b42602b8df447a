"""Body-part segmentation on the MI355X (include/hnrf_segment.h, csrc/hnrf_segment.hip): the member words and the
compaction against the numpy twin of humannerf_amd/cloud.py -- held to the reference's own loop by
tests/test_segment_refs.py -- bit for bit.  No tolerance anywhere: integer arithmetic and selection; the fused
matrices are compared with the per-part route on the same device, where both hand hnrf_cloud_distance_pairs the same
clouds."""
import os

import numpy as np
import pytest
import torch

from humannerf_amd import cloud, ops
from humannerf_amd._lib import HnrfError

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 255, 256, 257, 1000)          # one batch: block edges, an empty frame first, frames that share blocks
PARTS = {1: {'only': [3, 15]}, 15: None, 32: dict({'p%02d' % p: [p % 24] for p in range(31)}, p31=[23, 5])}


def frames_of(H, W, counts=COUNTS, seed=0):
    """Random records: pixels drawn with repetition (shared pixels), bones 0 .. 23, weights on both sides of 0.3."""
    rs = np.random.RandomState(seed)
    out = []
    for n in counts:
        rec = np.concatenate([rs.uniform(0, 1, (n, 6)), rs.uniform(0.05, 1.0, (n, 1)), rs.randint(0, H, (n, 1)),
                              rs.randint(0, W, (n, 1)), rs.randint(0, 24, (n, 1))], axis=1).astype(np.float32)
        out.append(rec)
    return out


def pack(frames):
    rec = torch.from_numpy(np.concatenate(frames) if frames else np.zeros((0, 10), np.float32)).to(DEV)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum([f.shape[0] for f in frames])]).astype(np.int64), device=DEV)
    return rec, offsets


def dev_masks(parts):
    masks = cloud.bone_masks(parts)
    return masks, torch.from_numpy(masks.view(np.int32)).to(DEV)


def device_segments(frames, parts, H, W, radius, weight_min=None, **kw):
    """-> member (uint32), seg_offsets, src as numpy, from the three entries."""
    rec, offsets = pack(frames)
    masks, dmasks = dev_masks(parts)
    member, status = ops.segment_members(rec, offsets, dmasks, H, W, radius, **kw)
    P = len(cloud.BODY_PARTS if parts is None else parts)
    seg, src = ops.segment_compact(member, offsets, P, status=status, weight_rec=None if weight_min is None else rec,
                                   weight_min=0.0 if weight_min is None else weight_min)
    return member.cpu().numpy().view(np.uint32), seg.numpy(), src.cpu().numpy()


def twin_segments(frames, parts, H, W, radius, weight_min=None):
    masks = cloud.bone_masks(parts)
    members = [cloud.twin_segment(f, masks, H, W, radius) for f in frames]
    P = len(cloud.BODY_PARTS if parts is None else parts)
    seg, src = cloud.twin_compact(members, P, weights=None if weight_min is None else [f[:, 6] for f in frames],
                                  weight_min=0.0 if weight_min is None else weight_min)
    return (np.concatenate(members) if members else np.zeros(0, np.uint32)), seg, src


def assert_same(got, want):
    for g, w, what in zip(got, want, ('member', 'seg_offsets', 'src')):
        assert g.dtype == w.dtype and np.array_equal(g, w), what


@pytest.fixture(scope='module')
def golden_records():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'segments.npz'))
    return {str(n): torch.from_numpy(g['seg/rec/%s' % n]) for n in g['seg/frames']}


def test_golden_frames_equal_the_twin(golden_records):
    frames = [r.numpy() for r in golden_records.values()]
    got = device_segments(frames, None, 40, 56, 10)
    assert_same(got, twin_segments(frames, None, 40, 56, 10))
    assert got[1][-1] == got[2].size > 0


@pytest.mark.parametrize('n_parts', [1, 15, 32])
@pytest.mark.parametrize('radius', [1, 10, 33])
@pytest.mark.parametrize('size', [(40, 56), (7, 300)], ids=str)
def test_members_and_compaction_equal_the_twin(size, radius, n_parts):
    H, W = size
    frames = frames_of(H, W)
    got = device_segments(frames, PARTS[n_parts], H, W, radius)
    want = twin_segments(frames, PARTS[n_parts], H, W, radius)
    assert_same(got, want)
    if n_parts == 32:
        assert (got[0] >> np.uint32(31)).any() and not (got[0] >> np.uint32(31)).all()      # bit 31 is in use


def test_batches_of_frames_and_two_runs_give_equal_bytes():
    frames = frames_of(40, 56)
    one = device_segments(frames, None, 40, 56, 10)
    again = device_segments(frames, None, 40, 56, 10)
    for a, b in zip(one, again):
        assert a.tobytes() == b.tobytes()
    for per in (1, 4):                                                    # the host's split of a long run
        assert_same(device_segments(frames, None, 40, 56, 10, frames_per_batch=per), one)
    # no frames, and frames without records
    assert_same(device_segments([], None, 40, 56, 10), twin_segments([], None, 40, 56, 10))
    empty = [np.zeros((0, 10), np.float32)] * 3
    assert_same(device_segments(empty, None, 40, 56, 10), twin_segments(empty, None, 40, 56, 10))


def test_the_weight_predicate_drops_rows_at_or_below_the_threshold():
    frames = frames_of(40, 56, seed=4)
    thr = np.float32(0.3)
    frames[3][:40, 6] = thr                                               # exactly the threshold: dropped
    frames[3][40:80, 6] = np.nextafter(thr, np.float32(1))                # one ulp above: kept
    frames[4][5, 6] = np.nan                                              # never kept
    got = device_segments(frames, None, 40, 56, 10, weight_min=float(thr))
    assert_same(got, twin_segments(frames, None, 40, 56, 10, weight_min=float(thr)))
    everything = device_segments(frames, None, 40, 56, 10)
    w = np.concatenate(frames)[:, 6]
    assert (w[got[2]] > thr).all()
    dropped = np.setdiff1d(everything[2], got[2])
    assert dropped.size and not (w[dropped] > thr).any()
    kept_all = everything[2][w[everything[2]] > thr]
    assert np.array_equal(kept_all, got[2])                               # exactly the rows above it, in order


def test_a_bad_record_raises_and_nothing_is_written():
    frames = frames_of(40, 56, counts=(300, 200))
    for column, value, bit in ((7, 40.0, 2), (8, -1.0, 2), (7, 2.5, 1), (8, float('nan'), 1), (9, 0.5, 4)):
        bad = [f.copy() for f in frames]
        bad[1][17, column] = value
        rec, offsets = pack(bad)
        member = torch.full((500,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
        _, status = ops.segment_members(rec, offsets, dev_masks(None)[1], 40, 56, 10, member=member)
        assert int(status.cpu()[0]) == bit and (member.cpu().numpy() == 0x5a5a5a5a).all()
        with pytest.raises(HnrfError):
            ops.segment_compact(member, offsets, 15, status=status)
        with pytest.raises(HnrfError):
            cloud.segment_records({'a': torch.from_numpy(bad[0]), 'b': torch.from_numpy(bad[1])}, image_size=(40, 56))
    # the image the records themselves span holds every one of them
    assert cloud.segment_records({'a': torch.from_numpy(frames[0])})['head']['a'] is not None


def test_segment_records_and_fused_matrices(golden_records):
    rs = np.random.RandomState(5)
    recs = dict(golden_records)
    for k in range(3):
        r = golden_records['f000_big'].numpy().copy()[rs.permutation(700)[:300 + 100 * k]]
        r[:, :3] += rs.uniform(-0.004, 0.004, r[:, :3].shape).astype(np.float32)
        assert np.unique(r[:, 1]).size == r.shape[0]
        recs['g%03d' % k] = torch.from_numpy(r)
    recs['h_none'] = None
    seg = cloud.segment_records(recs, image_size=(40, 56))
    twin = cloud.segment_records(recs, image_size=(40, 56), backend='twin')
    for part in cloud.BODY_PARTS:
        for name in recs:
            a, b = seg[part][name], twin[part][name]
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), (part, name)
    fused = cloud.segment_distance_matrices(recs, image_size=(40, 56), dist_thresh=0.03, axis=1)
    busy = 0
    for part in cloud.BODY_PARTS:
        want = cloud.distance_matrix(seg[part], dist_thresh=0.03, axis=1)
        assert fused[part].dtype == np.float32 and np.array_equal(fused[part], want), part
        busy += bool(want.any())
    assert busy >= 6
    chunk = cloud.segment_distance_matrices(recs, image_size=(40, 56), dist_thresh=0.03, axis=1, chunk=(1, 3),
                                            pairs_per_launch=7)
    rows = cloud.chunk_rows(len(recs), (1, 3))
    for part in ('head', 'belly'):
        keep = np.zeros_like(fused[part], dtype=bool)
        for i in rows:
            keep[i, i + 1:] = True
        assert np.array_equal(chunk[part], np.where(keep | keep.T, fused[part], 0))


def test_records_to_clusters_in_one_session(seeded_params, golden_dir, tmp_path):
    """run_surface_points -> run_segments -> run_segment_distance_matrices -> run_cluster leaves the reference's tree."""
    import pickle
    from humannerf_amd import dataset, run
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network
    net = Network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_params.items()}, strict=True)
    net = net.to(DEV).eval()
    subj = dataset.Subject(os.path.join(golden_dir, 'subject_synth'))
    old = (cfg.amd.diagnostics, cfg.N_samples, cfg.bgcolor)
    cfg.amd.diagnostics, cfg.N_samples, cfg.bgcolor = False, 64, [255., 255., 255.]
    try:
        res = run.run_surface_points(net, subj, weight_threshold=0.01, logdir=str(tmp_path))
    finally:
        cfg.amd.diagnostics, cfg.N_samples, cfg.bgcolor = old
    out = tmp_path / 'latest'
    records = torch.load(res['path'])
    seg = run.run_segments(res['path'])
    twin = cloud.segment_records(records, backend='twin')
    present = 0
    for part in cloud.BODY_PARTS:
        assert seg['paths'][part] == str(out / ('name-2-3d.%s.bin' % part))
        back = torch.load(seg['paths'][part])
        for name in records:
            a, b = back[name], twin[part][name]
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), (part, name)
            present += a is not None
    assert present > 0
    mats = run.run_segment_distance_matrices(res['path'], valid_weight_threshold=0.3, dist_thresh=0.002, axis=1)
    for part in cloud.BODY_PARTS:
        path = out / 'distance_mat_seg' / part / 'distance_mat_0.30-0.00.npy'
        assert mats['paths'][part] == str(path) and np.load(path).shape == (3, 3)
    wide = run.run_segment_distance_matrices(records, valid_weight_threshold=0.01, dist_thresh=0.02, axis=1,
                                             out_dir=str(tmp_path / 'wide'))
    for part, D in wide['matrices'].items():                              # (bit parity of the two routes: the test above)
        assert wide['paths'][part] == str(tmp_path / 'wide' / 'distance_mat_seg' / part / 'distance_mat_0.01-0.02.npy')
        assert D.shape == (3, 3) and np.array_equal(D, D.T) and not D.diagonal().any()
    got = run.run_cluster(mats['paths']['head'], names=mats['names'], n_clusters=1)
    assert got['path'] == str(out / 'distance_mat_seg' / 'head' / 'distance_mat_0.30-0.00.cluster.pkl')
    with open(got['path'], 'rb') as f:
        assert pickle.load(f) == got['clusters'] and sorted(got['clusters'][0]['names']) == sorted(records)
