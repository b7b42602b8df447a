"""Surface points and the frame distance on the MI355X (include/hnrf_cloud.h, csrc/hnrf_cloud.hip): every kernel against
the numpy twin of humannerf_amd/cloud.py -- held to the reference's own functions by tests/test_cloud_refs.py -- bit for
bit where the statement fixes the bits (nearest neighbours, d2, partners, the surface points' fixed summation order),
and against fp64 where it fixes a bound.

Bounds.  D is the fp64 sum of fp32 colour errors that are the twin's bit for bit; only the order of at most ~700 fp64
additions of non-negative terms differs (workgroup partials against numpy's pairwise sum): 1e-12 relative covers
700 * 2^-53 = 8e-14.  wxyz: within 4 x the error that the reference's fp32 expression (torch.sum(w[..., None] * xyz, 1)
on the host) makes on the same inputs against fp64, the convention of the render-kernel tests."""
import os

import numpy as np
import pytest
import torch

from humannerf_amd import cloud, ops
from humannerf_amd._lib import HnrfError

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BOX = np.array([0.09, 0.18, 0.03])


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tie_lattice(rs):
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), indexing='ij'), -1).reshape(-1, 2)
    a = np.concatenate([g, np.zeros((g.shape[0], 1))], 1).astype(np.float32)
    b = (a + np.float32([0.5, 0.5, 0.0]))[rs.permutation(a.shape[0])]
    return a, b


# ------------------------------------------------------------------------------------------------ hnrf_cloud_nn
NN_SHAPES = [(1, 1), (1, 257), (63, 64), (64, 65), (257, 1), (300, 1000), (5, 0), (0, 5), 'lattice', (1000, 2500)]


@pytest.mark.parametrize('shape', NN_SHAPES, ids=str)
def test_cloud_nn_equals_the_twin_bit_for_bit(shape):
    rs = np.random.RandomState(17)
    if shape == 'lattice':
        a, b = tie_lattice(rs)
    else:
        a = (rs.uniform(0, 1, (shape[0], 3)) * BOX).astype(np.float32)
        b = (rs.uniform(0, 1, (shape[1], 3)) * BOX).astype(np.float32)
        b[::7] = np.round(b[::7] * 64) / 64                               # duplicates: equal d2 at different indices
    Na = a.shape[0]
    idx = torch.full((Na + 9,), -7777, dtype=torch.int32, device=DEV)
    d2 = torch.full((Na + 9,), float('nan'), device=DEV)
    ops.cloud_nn(T(a), T(b), idx=idx, d2=d2)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert (idx[Na:] == -7777).all() and np.isnan(d2[Na:]).all()           # nothing written past Na
    pos, want = cloud.twin_nn(a, b)
    assert np.array_equal(idx[:Na], pos)
    assert np.array_equal(bits(d2[:Na]), bits(want))
    if b.shape[0] == 0:
        assert (idx[:Na] == -1).all() and np.isposinf(d2[:Na]).all()
    if shape == 'lattice':
        assert (d2[:Na] == 0.5).all()                                     # four exact ties each: the lowest index won


def test_nearest_pairs_public_form():
    rs = np.random.RandomState(4)
    x0 = (rs.uniform(0, 1, (300, 3)) * BOX).astype(np.float32)
    x1 = (x0[:200] + rs.normal(0, 1, (200, 3)) * 1e-3).astype(np.float32)[rs.permutation(200)]
    got = [t.cpu().numpy() for t in cloud.nearest_pairs(x0, x1, device=DEV)]
    want = cloud.twin_nearest_pairs(x0, x1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].size > 50
    assert np.allclose(got[2], want[2], rtol=1e-6) and np.allclose(got[3], want[3], rtol=1e-6)
    p0, p1, d01, d10 = cloud.nearest_pairs(x0, x1, dist_thresh=0.002, device=DEV)
    t0, t1, _, _ = cloud.nearest_pairs(x0, x1, dist_thresh=0.002, backend='twin')
    assert d01 is None and d10 is None
    assert np.array_equal(p0.cpu().numpy(), t0) and np.array_equal(p1.cpu().numpy(), t1) and 0 < t0.size < want[0].size


# ------------------------------------------------------------------------------------ hnrf_cloud_distance_pairs
COUNTS = [0, 1, 64, 257, 700]
PAIRS = [(i, j) for i in range(5) for j in range(i + 1, 5)]


@pytest.fixture(scope='module')
def five_frames():
    """Frames of 0, 1, 64, 257 and 700 points: noisy subsets of one base cloud, a quarter snapped to a lattice (exact
    ties and duplicates), with colours.  Unsorted: the record order."""
    rs = np.random.RandomState(23)
    base = rs.uniform(0, 1, (700, 3)) * BOX
    frames = []
    for n in COUNTS:
        x = base[rs.permutation(700)[:n]] + rs.normal(0, 1, (n, 3)) * 6e-4
        snap = rs.rand(n) < 0.25
        x[snap] = np.round(x[snap] * 512) / 512
        frames.append((x.astype(np.float32), rs.rand(n, 3).astype(np.float32)))
    return frames


def _packed(frames, axis):
    pk = cloud._pack([T(x) for x, _ in frames], axis, DEV, colours=[T(c) for _, c in frames])
    assert pk['max_n'] == 700
    return pk


def _run(pk, pairs, tau, axis, want_match=True):
    D, match = ops.cloud_distance_pairs(pk['xyz'], pk['rgb'], pk['orig'], pk['offsets'],
                                        torch.tensor(pairs, dtype=torch.int32, device=DEV), tau, axis, pk['max_n'],
                                        want_match=want_match)
    return D.cpu().numpy(), None if match is None else match.cpu().numpy()


@pytest.mark.parametrize('axis', [0, 1, 2])
@pytest.mark.parametrize('tau', [0.002, 0.05, 10.0])
def test_distance_pairs_against_twin_and_brute_force(five_frames, tau, axis):
    pk = _packed(five_frames, axis)
    D, match = _run(pk, PAIRS, tau, axis)
    off = pk['offsets'].cpu().numpy()
    orig = pk['orig'].cpu().numpy()
    sorted_frames = [cloud.sort_frame(x, c, axis) for x, c in five_frames]
    n_pairs = 0
    for k, (i, j) in enumerate(PAIRS):
        ni = COUNTS[i]
        # the device's torch.sort may order equal keys differently from numpy's: compare per ORIGINAL record
        got = np.full(ni, -1, np.int64)
        got[orig[off[i]:off[i + 1]]] = match[k, :ni]
        assert (match[k, ni:] == -1).all()
        tm, terr, tD = cloud.twin_pairs(sorted_frames[i], sorted_frames[j], tau, axis)
        want = np.full(ni, -1, np.int64)
        want[sorted_frames[i]['orig']] = tm
        assert np.array_equal(got, want), (i, j)
        # ... and the composition of two brute-force launches on the unsorted records
        a, b = T(five_frames[i][0]), T(five_frames[j][0])
        if ni and COUNTS[j]:
            m0, d2 = (t.cpu().numpy() for t in ops.cloud_nn(a, b))
            m1 = ops.cloud_nn(b, a)[0].cpu().numpy()
            mutual = (m1[m0] == np.arange(ni)) & (np.sqrt(d2) < np.float32(tau))
            assert np.array_equal(got, np.where(mutual, m0, -1)), (i, j)
        ref = float(np.sum(terr.astype(np.float64)))
        print('tau %g axis %d pair %s: %d pairs, D %.17g twin %.17g' % (tau, axis, (i, j), (tm >= 0).sum(), D[k], ref))
        assert abs(D[k] - ref) <= 1e-12 * abs(ref)
        n_pairs += int((tm >= 0).sum())
    assert n_pairs > (30 if tau < 0.01 else 300)
    # reproducible, a function of the pair alone, and symmetric in the pair
    D2, match2 = _run(pk, PAIRS, tau, axis)
    assert np.array_equal(D2.view(np.uint64), D.view(np.uint64)) and np.array_equal(match2, match)
    perm = np.random.RandomState(1).permutation(len(PAIRS))
    Dp, _ = _run(pk, [PAIRS[p] for p in perm], tau, axis, want_match=False)
    assert np.array_equal(Dp.view(np.uint64), D[perm].view(np.uint64))
    Dr, mr = _run(pk, [(j, i) for i, j in PAIRS], tau, axis)
    for k, (i, j) in enumerate(PAIRS):
        fwd = {(int(o), int(m)) for o, m in zip(orig[off[i]:off[i + 1]], match[k, :COUNTS[i]]) if m >= 0}
        bwd = {(int(m), int(o)) for o, m in zip(orig[off[j]:off[j + 1]], mr[k, :COUNTS[j]]) if m >= 0}
        assert fwd == bwd
        assert abs(Dr[k] - D[k]) <= 1e-12 * abs(D[k])


@pytest.mark.parametrize('tau', [float('nan'), float('inf'), 0.0, -0.002])
def test_distance_pairs_refuses_a_bad_threshold(five_frames, tau):
    pk = _packed(five_frames, 1)
    with pytest.raises(HnrfError, match='tau'):
        _run(pk, PAIRS, tau, 1)
    torch.cuda.synchronize()


def test_distance_matrix_on_the_device_equals_the_twin(five_frames):
    rs = np.random.RandomState(9)
    recs = {}
    for k, (x, c) in enumerate(five_frames):
        n = x.shape[0]
        recs['f%d' % k] = torch.from_numpy(np.concatenate(
            [x, c, rs.uniform(0.2, 1, (n, 1)), rs.randint(0, 64, (n, 2)), rs.randint(0, 24, (n, 1))], 1).astype(np.float32))
    recs['f5'] = None
    want = cloud.distance_matrix(recs, dist_thresh=0.002, backend='twin')
    for method in ('window', 'brute'):
        got = cloud.distance_matrix(recs, dist_thresh=0.002, method=method, device=DEV)
        assert np.array_equal(got, want) and np.count_nonzero(got) >= 6, method
    part = cloud.distance_matrix(recs, dist_thresh=0.002, chunk=(1, 2), device=DEV, pairs_per_launch=3)
    assert np.array_equal(part, cloud.distance_matrix(recs, dist_thresh=0.002, chunk=(1, 2), backend='twin'))
    d = cloud.frame_distance(recs['f3'], recs['f4'], dist_thresh=0.002, device=DEV)
    assert np.float32(d) == want[3, 4] and cloud.frame_distance(recs['f3'], None, device=DEV) == 0


# ------------------------------------------------------------------------------------------ hnrf_surface_points
def _rays(R, S, B, seed=0):
    """Weights with one peak per ray, per-sample bone weights peaked on one bone per ray (the same for the ray's
    samples, as neighbouring samples of a body part are): the blended weights have a clear winner."""
    g = torch.Generator().manual_seed(seed)
    w = torch.softmax(6 * torch.randn(R, S, generator=g), -1) * torch.rand(R, 1, generator=g)
    bone = torch.randint(0, B, (R, 1, 1), generator=g)
    logits = torch.randn(R, S, B, generator=g).scatter_add(2, bone.expand(R, S, 1), torch.full((R, S, 1), 4.0))
    return w.contiguous(), torch.randn(R, S, 3, generator=g), torch.softmax(logits, -1).contiguous()


SP_SHAPES = [(1, 2, 24), (7, 64, 24), (65, 128, 24), (33, 257, 24), (5, 128, 7), (3, 512, 32)]


@pytest.fixture(scope='module')
def surface_cases():
    """shape -> inputs, the kernel's outputs and the fp64 / fp32 host references, computed once."""
    out = {}
    for R, S, B in SP_SHAPES:
        w, xyz, bmw = _rays(R, S, B, seed=R)
        got = [t.cpu() for t in ops.surface_points(w.to(DEV), xyz.to(DEV), bmw.to(DEV))]
        ref64 = torch.sum(w.double()[..., None] * xyz.double(), axis=1)
        ref32 = torch.sum(w[..., None] * xyz, axis=1)
        out[(R, S, B)] = dict(w=w, xyz=xyz, bmw=bmw, got=got, ref64=ref64, ref32=ref32,
                              lbs64=torch.sum(w.double()[..., None] * bmw.double(), axis=1))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('shape', SP_SHAPES, ids=str)
def test_surface_points_kernel(surface_cases, shape):
    c = surface_cases[shape]
    wxyz, wmax, lbs = c['got']
    assert lbs.dtype == torch.int32
    err = float((wxyz.double() - c['ref64']).abs().max())
    bound = 4 * float((c['ref32'].double() - c['ref64']).abs().max())
    print(shape, 'wxyz err %.3g, 4 x the fp32 expression %.3g' % (err, bound))
    assert err <= bound
    assert torch.equal(wmax, c['w'].max(dim=1)[0])
    top2 = torch.topk(c['lbs64'], 2, dim=1)[0]
    decided = (top2[:, 0] - top2[:, 1]) > 1e-5 * top2[:, 0]
    assert float((~decided).float().mean()) <= 0.01
    ref32 = torch.argmax(torch.sum(c['w'][..., None] * c['bmw'], axis=1), dim=1)
    assert torch.equal(ref32[decided], torch.argmax(c['lbs64'], dim=1)[decided])     # (the fp32 expression meets the cap)
    assert torch.equal(lbs.long()[decided], torch.argmax(c['lbs64'], dim=1)[decided])
    # the documented order of the sums: the numpy twin has the same bits
    t_wxyz, t_wmax, t_lbs = cloud.twin_surface_points(c['w'].numpy(), c['xyz'].numpy(), c['bmw'].numpy())
    assert np.array_equal(bits(wxyz.numpy()), bits(t_wxyz)) and np.array_equal(lbs.numpy(), t_lbs)


def test_surface_points_lowest_index_and_batch_independence(surface_cases):
    # exactly equal columns: powers of two add without rounding, columns 3 and 7 hold the same, largest values
    R, S, B = 6, 128, 24
    g = torch.Generator().manual_seed(1)
    w = torch.pow(2.0, -torch.randint(1, 6, (R, S), generator=g).float())
    bmw = torch.pow(2.0, -torch.randint(4, 8, (R, S, B), generator=g).float())
    bmw[:, :, 3] = 0.5
    bmw[:, :, 7] = 0.5
    xyz = torch.randn(R, S, 3, generator=g)
    _, _, lbs = ops.surface_points(w.to(DEV), xyz.to(DEV), bmw.to(DEV))
    assert (lbs.cpu() == 3).all()
    bmw[:, :, 3] = 0.25
    assert (ops.surface_points(w.to(DEV), xyz.to(DEV), bmw.to(DEV))[2].cpu() == 7).all()
    # a ray alone = the same ray in a batch, bit for bit
    c = surface_cases[(65, 128, 24)]
    for r in (0, 3, 64):
        one = ops.surface_points(c['w'][r:r + 1].to(DEV), c['xyz'][r:r + 1].to(DEV), c['bmw'][r:r + 1].to(DEV))
        for a, b in zip(one, c['got']):
            assert torch.equal(a.cpu()[0], b[r])
    for bad in ((4, 513, 24), (4, 8, 33)):
        w, xyz, bmw = (torch.zeros(s, device=DEV) for s in (bad[:2], bad[:2] + (3,), bad))
        with pytest.raises(HnrfError, match='S <= 512'):
            ops.surface_points(w, xyz, bmw)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def gpu_net(seeded_params):
    from humannerf_amd.network import Network
    net = Network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_params.items()}, strict=True)
    return net.to(DEV).eval()


def test_surface_records_of_the_seeded_network(gpu_net, golden_frame):
    from humannerf_amd.config import cfg
    keys = ['rays', 'near', 'far', 'dst_Rs', 'dst_Ts', 'cnl_gtfms', 'motion_weights_priors', 'dst_posevec',
            'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor']
    data = {k: T(golden_frame[k]) for k in keys}
    old = (cfg.amd.diagnostics, cfg.N_samples, cfg.perturb)
    cfg.amd.diagnostics, cfg.N_samples, cfg.perturb = True, 128, 0.
    try:
        with torch.no_grad():
            out = gpu_net(**data, iter_val=1e7)
            cfg.amd.diagnostics = False
            lean = gpu_net(**data, iter_val=1e7)
    finally:
        cfg.amd.diagnostics, cfg.N_samples, cfg.perturb = old
    hit = np.asarray(golden_frame['ray_mask']).reshape(-1)
    W = int(round(np.sqrt(hit.size)))
    ray_index = torch.from_numpy(np.nonzero(hit)[0]).to(DEV)
    R = out['rgb'].shape[0]
    truth = torch.rand(R, 3, generator=torch.Generator().manual_seed(0)).to(DEV)
    wmax = out['weights_on_rays'].max(dim=1)[0]
    thr = float(wmax.median())
    rec = cloud.surface_records(out, truth, ray_index, W, thr)
    keep = wmax > thr
    assert rec.is_cuda and rec.dtype == torch.float32 and rec.shape == (int(keep.sum()), 10) and 0 < rec.shape[0] < R
    w, xyz, bmw = (out[k].double() for k in cloud.RECORD_KEYS)
    want_xyz = torch.sum(w[..., None] * xyz, axis=1)[keep]
    ref32 = torch.sum(out['weights_on_rays'][..., None] * out['xyz_on_rays'], axis=1)[keep].double()
    assert float((rec[:, :3].double() - want_xyz).abs().max()) <= 4 * float((ref32 - want_xyz).abs().max())
    assert torch.equal(rec[:, 3:6], truth[keep]) and torch.equal(rec[:, 6], wmax[keep])
    assert torch.equal(rec[:, 7].long() * W + rec[:, 8].long(), ray_index[keep])
    lbs = torch.sum(w[..., None] * bmw, axis=1)[keep]
    top2 = torch.topk(lbs, 2, dim=1)[0]
    decided = (top2[:, 0] - top2[:, 1]) > 1e-5 * top2[:, 0]
    assert torch.equal(rec[:, 9].long()[decided], torch.argmax(lbs, dim=1)[decided])
    with pytest.raises(HnrfError, match='diagnostics'):
        cloud.surface_records(lean, truth, ray_index, W, thr)


def test_run_surface_points_on_a_subject_directory(gpu_net, golden_dir, tmp_path):
    from humannerf_amd import dataset, run
    from humannerf_amd.config import cfg
    subj = dataset.Subject(os.path.join(golden_dir, 'subject_synth'))
    old = (cfg.amd.diagnostics, cfg.N_samples, cfg.bgcolor)
    cfg.amd.diagnostics, cfg.N_samples, cfg.bgcolor = False, 64, [255., 255., 255.]
    try:
        res = run.run_surface_points(gpu_net, subj, weight_threshold=0.01, logdir=str(tmp_path))
        assert cfg.amd.diagnostics is False                              # restored
    finally:
        cfg.amd.diagnostics, cfg.N_samples, cfg.bgcolor = old
    assert res['path'] == str(tmp_path / 'latest' / 'name-2-3d.bin') and res['frames'] == [0, 1, 2]
    got = torch.load(res['path'])
    assert sorted(got) == ['frame_000003', 'frame_000010', 'frame_000042']
    for name, rec in got.items():
        assert rec.device.type == 'cpu' and rec.dtype == torch.float32 and rec.dim() == 2 and rec.shape[1] == 10
        assert torch.equal(rec, res['records'][name])
        assert (rec[:, 6] > 0.01).all() and (rec[:, 7] < 64).all() and (rec[:, 8] < 48).all()
        assert ((rec[:, 9] >= 0) & (rec[:, 9] < 24)).all()
    assert sum(r.shape[0] for r in got.values()) > 0
    mat = run.run_distance_matrix(res['path'], valid_weight_threshold=0.01, dist_thresh=0.02, device=DEV)
    assert mat['path'] == str(tmp_path / 'latest' / 'distance_mat' / 'distance_mat_0.01-0.02.npy')
    assert mat['matrix'].shape == (3, 3) and np.array_equal(mat['matrix'], mat['matrix'].T)
    twin = cloud.distance_matrix(got, valid_weight_threshold=0.01, dist_thresh=0.02, backend='twin')
    assert np.array_equal(mat['matrix'], twin)
