"""The numpy twins of the skinned export's kernels (humannerf_amd/skin.py: skin_weights_host, skin_lbs_host,
joint_matrices) against fp64 statements, without a GPU; tests/test_gpu_skin.py then holds the kernels to the twins bit
for bit.  Problems: tests/test_mesh_kernel_refs.py (skin_problem over SKIN_CASES, skin_exact_problem).  Tolerances: the
rule of tests/test_gpu_mesh_kernels.py::_check -- 4 x the error of the reference's own fp32 evaluation against fp64.

The references and the helpers at the top are shared with the GPU tests (computed once per case)."""
import functools

import numpy as np
import pytest
import torch

from humannerf_amd import skin
from oracle import oracle
from tests import test_mesh_kernel_refs as mrefs
from tests import test_render_kernel_refs as refs
from tests.test_gpu_mesh_kernels import _check

KS = [4, 8]
CASE_IDS = lambda c: 'B%d_G%d_V%d' % c
MAX_EXEMPT = 0.01


# ------------------------------------------------------------------------------------------------ references
def ref_weights(pr, dtype=torch.float64):
    """w_b of every vertex (V, B) as mrefs.ref_skin samples it (oracle.trilinear_zeros), in ``dtype``."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    g = (t(pr['verts']) - t(pr['bmin'])) * t(pr['bscale']) - 1.0
    vol = t(pr['vol'])
    return torch.stack([oracle.trilinear_zeros(vol[b], g) for b in range(pr['B'])], -1)


def ref_topk(w, K):
    """The K largest positive weights of w (V, B), descending, ties to the lower bone: (values (V, K), joints (V, K),
    gaps (V, K) = value k minus the next value in the full order (the K-th: minus the (K+1)-th)), zero-padded."""
    w = np.asarray(w, dtype=np.float64)
    V, B = w.shape
    order = np.argsort(-w, axis=1, kind='stable')
    val = np.take_along_axis(w, order, 1)
    val = np.concatenate([np.where(val > 0, val, 0.0), np.zeros((V, K + 1))], 1)[:, :K + 1]
    jn = np.concatenate([order, np.zeros((V, K + 1), np.int64)], 1)[:, :K]
    jn = np.where(val[:, :K] > 0, jn, 0)
    return val[:, :K], jn, val[:, :K] - val[:, 1:K + 1]


@functools.lru_cache(maxsize=None)
def case_refs(case):
    """(problem, w64, w32) of a SKIN_CASES shape, computed once and shared."""
    pr = mrefs.skin_problem(*case)
    w64, w32 = ref_weights(pr).numpy(), ref_weights(pr, torch.float32).numpy()
    return pr, w64, w32                                  # (read, never written)


def host_weights(pr, K):
    return skin.skin_weights_host(pr['verts'], pr['vol'], pr['bmin'], pr['bscale'], k=K, n_bones=pr['B'])


def check_topk(tag, case, K, joints, weights, kept):
    """The comparison of one (joints, weights, kept) with the fp64 top-K, for the twins here and the kernels on the
    GPU."""
    pr, w64, w32 = case_refs(case)
    v64, j64, gap = ref_topk(w64, K)
    v32, _, _ = ref_topk(w32, K)
    tol, _ = refs.tolerance(v32, v64)
    got = weights.astype(np.float64) * kept.astype(np.float64)[:, None]
    _check(tag + ' weights x kept', got, torch.from_numpy(v64), torch.from_numpy(v32))
    # the selection is decided where the K-th and the (K+1)-th weight are further apart than the tolerance; the order
    # inside it where every neighbouring pair of the selected ones is (pairs of zeros: padded slots, nothing to decide)
    undecided = ((gap <= tol) & (v64 > 0)).any(1)
    set_undecided = (gap[:, K - 1] <= tol) & (v64[:, K - 1] > 0)
    print('RATIO %s tol %.3e exempt %.4f (selection alone %.4f)' % (tag, tol, undecided.mean(), set_undecided.mean()))
    # at most 1 % of a case may be exempt from the selection; the order has K pairs to be close in, not one
    assert set_undecided.mean() <= MAX_EXEMPT and undecided.mean() <= K * MAX_EXEMPT, (tag, undecided.mean())
    assert np.array_equal(joints[~undecided].astype(np.int64), j64[~undecided]), tag
    rows = ~set_undecided & (kept > 0)                   # (no weight at all: (joint 0, weight 1), check_rows)
    assert all(set(a[m]) == set(b[n]) for a, m, b, n in
               zip(joints[rows].astype(np.int64), weights[rows] > 0, j64[rows], v64[rows] > 0)), tag
    check_rows(joints, weights, kept)


def check_rows(joints, weights, kept):
    """What glTF asks of every row: weights >= 0 and summing to 1, no joint twice with a non-zero weight, padded slots
    (joint 0, weight 0); and this package's rule for a vertex with no weight."""
    assert joints.dtype == np.uint8 and weights.dtype == np.float32 and kept.dtype == np.float32
    assert (weights >= 0).all() and np.abs(weights.astype(np.float64).sum(1) - 1).max() <= 4 * 2.0 ** -23
    assert (np.diff(weights.astype(np.float64), axis=1) <= 0).all()                  # descending
    assert (joints[weights == 0] == 0).all()
    for row_j, row_w in zip(joints[(weights > 0).sum(1) > 1], weights[(weights > 0).sum(1) > 1]):
        live = row_j[row_w > 0]
        assert len(set(live.tolist())) == len(live)
    none = kept == 0
    assert (joints[none] == 0).all() and (weights[none, 0] == 1).all() and (weights[none, 1:] == 0).all()


# ------------------------------------------------------------------------------------------------ the twins
def test_twin_samples_the_weights_of_forward_skin():
    """bone_weights_host against the fp64 sampling of mrefs.ref_skin, on the largest case."""
    case = mrefs.SKIN_CASES[4]
    pr, w64, w32 = case_refs(case)
    w = skin.bone_weights_host(pr['verts'], pr['vol'], pr['bmin'], pr['bscale'], n_bones=pr['B'])
    assert w.dtype == np.float32 and (w[pr['all_out']] == 0).all()
    _check('skin-twin w B%d G%d V%d' % case, w, torch.from_numpy(w64), torch.from_numpy(w32))


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('case', mrefs.SKIN_CASES, ids=CASE_IDS)
def test_twin_against_fp64_top_k(case, K):
    pr, _, _ = case_refs(case)
    joints, weights, kept = host_weights(pr, K)
    assert joints.shape == weights.shape == (pr['V'], K) and kept.shape == (pr['V'],)
    check_topk('skin-twin K%d B%d G%d V%d' % ((K,) + case), case, K, joints, weights, kept)
    out = pr['all_out']
    assert (kept[out] == 0).all() and (kept[~out] > 0).all()
    if pr['B'] < K:
        assert (joints[:, pr['B']:] == 0).all() and (weights[:, pr['B']:] == 0).all()


# ------------------------------------------------------------------------------------------------ planted cases
def planted_problems():
    """name -> (verts, vol, bmin, bscale, B): the planted cases of the issue, shared with the GPU tests."""
    rs = np.random.RandomState(5)
    bmin, bscale = mrefs.SKIN_BMIN, (2.0 / mrefs.SKIN_EXTENT).astype(np.float32)
    inside = (bmin.astype(np.float64) + rs.uniform(0.05, 0.95, (300, 3)) * mrefs.SKIN_EXTENT).astype(np.float32)
    out = {}
    out['equal'] = (inside, np.full((25, 5, 5, 5), 0.03125, np.float32), bmin, bscale, 24)
    for B in (1, 3, 7):
        vol = rs.uniform(0.01, 1.0 / (B + 1), (B + 1, 4, 4, 4)).astype(np.float32)
        out['few-%d' % B] = (inside, vol, bmin, bscale, B)
    padded = inside.copy()
    padded[:100, 0] += 2 * mrefs.SKIN_EXTENT[0]                                          # a whole box outside on x
    padded[100:200, 1] = np.nan
    padded[200:, :] = np.nan
    padded[250:, 2] = np.inf
    out['padded'] = (padded, rs.uniform(0.01, 0.03, (25, 6, 6, 6)).astype(np.float32), bmin, bscale, 24)
    zero = rs.uniform(0.01, 0.03, (9, 3, 3, 3)).astype(np.float32)
    zero[:8] = 0
    out['zero-volume'] = (inside, zero, bmin, bscale, 8)
    return out


@pytest.mark.parametrize('K', KS)
def test_planted_cases_on_the_twin(K):
    pl = planted_problems()
    call = lambda name: skin.skin_weights_host(*pl[name][:4], k=K, n_bones=pl[name][4])
    joints, weights, kept = call('equal')
    assert (joints == np.arange(K)[None]).all() and (weights == weights[:, :1]).all() and (kept > 0).all()
    assert np.abs(weights - 1.0 / K).max() <= 2.0 ** -23
    for B in (1, 3, 7):
        joints, weights, kept = call('few-%d' % B)
        n = min(B, K)
        assert (weights[:, :n] > 0).all() and (weights[:, n:] == 0).all() and (joints[:, n:] == 0).all()
        assert all(sorted(r.tolist()) == list(range(n)) for r in joints[:, :n]) if B <= K else (joints < B).all()
        check_rows(joints, weights, kept)
    for name in ('padded', 'zero-volume'):
        joints, weights, kept = call(name)
        assert (kept == 0).all() and (joints == 0).all() and (weights[:, 0] == 1).all() and (weights[:, 1:] == 0).all()


def exact_statement(pr, lat, K):
    """hnrf_skin_weights on a problem of mrefs.skin_exact_problem, by hand: the weights are exact multiples of 2^-16
    below 1 in fp64, so is every partial sum of them; the order is a stable sort; one rounded division each."""
    w = refs.exact_lattice_weights(pr['vol'][:pr['B']], lat)
    val, jn, _ = ref_topk(w, K)
    kept = np.zeros(len(w))
    for k in range(K):
        kept = kept + val[:, k]
    assert np.array_equal(kept.astype(np.float32).astype(np.float64), kept)
    ok = kept > 0
    unit = np.zeros((len(w), K), np.float32)
    unit[:, 0] = 1
    with np.errstate(invalid='ignore', divide='ignore'):
        weights = np.where(ok[:, None], val.astype(np.float32) / kept.astype(np.float32)[:, None], unit)
    return np.where(ok[:, None], jn, 0).astype(np.uint8), weights.astype(np.float32), kept.astype(np.float32)


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('B', [24, 7])
def test_twin_on_the_exact_lattice_bit_for_bit(B, K):
    pr, lat = mrefs.skin_exact_problem(B)
    joints, weights, kept = host_weights(pr, K)
    j0, w0, k0 = exact_statement(pr, lat, K)
    assert np.array_equal(kept.view(np.uint32), k0.view(np.uint32))
    assert np.array_equal(joints, j0) and np.array_equal(weights.view(np.uint32), w0.view(np.uint32))
    assert (kept == 0).sum() > 1000 and (kept > 0).sum() > 1000
    ties = (np.diff(np.sort(refs.exact_lattice_weights(pr['vol'][:B], lat), axis=1)[:, ::-1][:, :K + 1], axis=1) == 0)
    assert (ties.any(1) & (kept > 0)).sum() > 100                   # exact ties are decided, by the bone index
    check_rows(joints, weights, kept)


# ------------------------------------------------------------------------------------------------ skinning
@pytest.mark.parametrize('case', [c for c in mrefs.SKIN_CASES if c[0] <= 8], ids=CASE_IDS)
def test_lbs_of_all_the_bones_is_the_forward_skin(case):
    """K = 8 >= B: nothing is truncated, and skin_lbs_host with joint_matrices of the problem's bases is ref_skin's
    out wherever the weight sum is not clamped (sum w >= 1e-2: the set the GPU test of hnrf_forward_skin compares)."""
    pr, _, _ = case_refs(case)
    assert pr['B'] in (1, 7)
    joints, weights, kept = host_weights(pr, 8)
    mats = skin.joint_matrices(pr['Rs'], pr['Ts'])
    assert mats.dtype == np.float32 and mats.shape == (pr['B'], 3, 4)
    out = skin.skin_lbs_host(pr['verts'], joints, weights, mats)
    r64, r32 = mrefs.ref_skin(pr), mrefs.ref_skin(pr, torch.float32)
    ok = r64['wsum'] >= 1e-2
    assert float(ok.double().mean()) >= mrefs.SKIN_MIN_SHARE
    _check('skin-lbs-twin B%d G%d V%d out' % case, out, r64['out'], r32['out'], sel=ok[:, None].expand(-1, 3))
    _check('skin-lbs-twin B%d G%d V%d kept' % case, kept, r64['wsum'], r32['wsum'])


def test_joint_matrices_invert_the_basis_in_fp64():
    pr, _, _ = case_refs(mrefs.SKIN_CASES[2])
    mats = skin.joint_matrices(pr['Rs'], pr['Ts'])
    R, T = pr['Rs'].astype(np.float64), pr['Ts'].astype(np.float64)
    inv = np.linalg.inv(R)
    want = np.concatenate([inv, -(inv @ T[:, :, None])], axis=2)
    assert np.array_equal(mats, want.astype(np.float32)) or np.abs(mats - want).max() <= 2.0 ** -23 * np.abs(want).max()
    tm = skin.joint_matrices(torch.from_numpy(pr['Rs']), torch.from_numpy(pr['Ts']))
    assert tm.dtype == torch.float32 and np.array_equal(tm.numpy(), mats)


def test_lbs_skips_a_joint_past_the_table():
    v = np.array([[0.1, 0.2, 0.3]], np.float32)
    mats = np.tile(np.concatenate([np.eye(3), np.ones((3, 1))], 1).astype(np.float32), (2, 1, 1))
    joints = np.array([[0, 1, 2, 255]], np.uint8)
    weights = np.array([[0.5, 0.25, 0.125, 0.125]], np.float32)
    out = skin.skin_lbs_host(v, joints, weights, mats)
    assert np.array_equal(out, ((v + 1) * np.float32(0.5) + (v + 1) * np.float32(0.25)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the binding
def test_the_entries_are_bound_beside_the_five_groups(monkeypatch):
    """The two entries live in include/hnrf_skin.h and a table of their own: GROUPS, _bind and the signatures of
    hnrf.h stay what they were; a library without the symbols raises the rebuild message from load_skin alone; and
    build() binds them after load_all()."""
    import subprocess

    import __graft_entry__ as entry
    from humannerf_amd import _lib
    sigs = _lib.SKIN_SIGNATURES
    assert set(sigs) == {'hnrf_skin_weights', 'hnrf_skin_lbs'} and not set(sigs) & set(_lib.SIGNATURES)
    assert 'skin' not in _lib.GROUPS and list(_lib.LATE_GROUPS) == ['skin']
    assert _lib.SKIN_HEADER_PATH.replace('\\', '/').endswith('/include/hnrf_skin.h')
    assert sigs['hnrf_skin_lbs'][1][1] is _lib.ctypes.c_int64 and sigs['hnrf_skin_weights'][1][7] is _lib.ctypes.c_int
    with pytest.raises(_lib.HnrfError) as e:
        _lib.load_skin(type('OldLib', (), {})())
    assert str(e.value) == ('%s does not export %s: it was built before the skinned glTF export (include/hnrf_skin.h); '
                            'rebuild it' % (_lib.LIB_PATH, next(iter(sigs))))
    late, early = [], []
    real_late, real = _lib._bind_late, _lib._bind
    monkeypatch.setattr(_lib, '_bind_late', lambda group, lib=None: late.append(group) or real_late(group, lib))
    monkeypatch.setattr(_lib, '_bind', lambda group, lib=None: early.append(group) or real(group, lib))
    monkeypatch.setattr(subprocess, 'run', lambda *a, **kw: None)          # (the library is built: no make)
    entry.build()
    assert late == ['skin'] and sorted(early) == sorted(_lib.GROUPS)
