"""The skinned glTF export on the MI355X: hnrf_skin_weights and hnrf_skin_lbs against their numpy twins BIT FOR BIT
(humannerf_amd/skin.py; the twins against fp64: tests/test_skin_refs.py, no GPU), run.run_gltf end to end -- the file
re-posed by an independent walker (tests/gltf_walker.py) against the device's own skinning -- and the binding of the
entries (a library without them).  hnrf_forward_skin itself is pinned by tests/test_gpu_mesh_kernels.py, unchanged."""
import numpy as np
import pytest
import torch

from humannerf_amd import skin
from tests import gltf_walker as walker
from tests import test_mesh_kernel_refs as mrefs
from tests import test_skin_refs as srefs
from tests.test_gpu_mesh_kernels import _check

pytestmark = pytest.mark.gpu
KS = srefs.KS


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def device_weights(verts, vol, bmin, bscale, B, K):
    out = skin.skin_weights(T(verts), T(vol), T(bmin), T(bscale), k=K, n_bones=B)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def same_bits(tag, got, want):
    for name, g, w in zip(('joints', 'weights', 'kept'), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
        bad = np.argwhere(bits(g) != bits(w))
        assert len(bad) == 0, (tag, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('case', mrefs.SKIN_CASES, ids=srefs.CASE_IDS)
def test_kernels_equal_their_twins_bit_for_bit(case, K):
    """Every SKIN_CASES shape (B = 1 .. 128, G = 2 .. 33, V = 1 .. 1000: one thread to four blocks, the last ragged):
    joints, weights and kept of hnrf_skin_weights, then hnrf_skin_lbs of those weights under the problem's bases."""
    pr, _, _ = srefs.case_refs(case)
    tag = 'skin K%d B%d G%d V%d' % ((K,) + case)
    want = srefs.host_weights(pr, K)
    got = device_weights(pr['verts'], pr['vol'], pr['bmin'], pr['bscale'], pr['B'], K)
    same_bits(tag, got, want)
    srefs.check_topk(tag, case, K, *got)
    mats = skin.joint_matrices(pr['Rs'], pr['Ts'])
    dmats = skin.joint_matrices(T(pr['Rs']), T(pr['Ts']))
    assert np.array_equal(bits(dmats.cpu().numpy()), bits(mats))
    out = skin.skin_lbs(T(pr['verts']), T(got[0]), T(got[1]), dmats)
    torch.cuda.synchronize()
    with np.errstate(all='ignore'):
        host = skin.skin_lbs_host(pr['verts'], want[0], want[1], mats)
    assert np.array_equal(bits(out.cpu().numpy()), bits(host)), tag


@pytest.mark.parametrize('K', KS)
def test_planted_cases_and_no_vertices(K):
    """The planted cases of tests/test_skin_refs.py (all channels equal, B < K, every corner padded, NaN and infinite
    coordinates, an all-zero volume) equal the twin bit for bit -- their values are asserted there -- and V = 0 returns
    empty tensors without a launch."""
    for name, (verts, vol, bmin, bscale, B) in srefs.planted_problems().items():
        want = skin.skin_weights_host(verts, vol, bmin, bscale, k=K, n_bones=B)
        got = device_weights(verts, vol, bmin, bscale, B, K)
        same_bits('planted %s K%d' % (name, K), got, want)
        mats = np.random.RandomState(B).uniform(-1, 1, (B, 3, 4)).astype(np.float32)
        out = skin.skin_lbs(T(verts), T(got[0]), T(got[1]), T(mats)).cpu().numpy()
        with np.errstate(all='ignore'):
            host = skin.skin_lbs_host(verts, want[0], want[1], mats)
        assert np.array_equal(np.isnan(out), np.isnan(host)) and np.array_equal(bits(out)[~np.isnan(out)], bits(host)[~np.isnan(host)])
    pr, _, _ = srefs.case_refs(mrefs.SKIN_CASES[2])
    empty = np.zeros((0, 3), np.float32)
    joints, weights, kept = device_weights(empty, pr['vol'], pr['bmin'], pr['bscale'], pr['B'], K)
    assert joints.shape == weights.shape == (0, K) and kept.shape == (0,)
    out = skin.skin_lbs(T(empty), T(joints), T(weights), T(skin.joint_matrices(pr['Rs'], pr['Ts'])))
    assert out.shape == (0, 3)


@pytest.mark.parametrize('B', [24, 7])
def test_exact_lattice_bit_for_bit_against_the_hand_statement(B):
    pr, lat = mrefs.skin_exact_problem(B)
    for K in KS:
        got = device_weights(pr['verts'], pr['vol'], pr['bmin'], pr['bscale'], B, K)
        same_bits('skin-exact B%d K%d' % (B, K), got, srefs.exact_statement(pr, lat, K))


def test_lbs_skips_a_joint_past_the_table_on_the_device():
    v = np.array([[0.1, 0.2, 0.3]] * 300, np.float32)
    mats = np.tile(np.concatenate([np.eye(3), np.ones((3, 1))], 1).astype(np.float32), (2, 1, 1))
    joints = np.array([[0, 1, 2, 255]] * 300, np.uint8)
    weights = np.array([[0.5, 0.25, 0.125, 0.125]] * 300, np.float32)
    out = skin.skin_lbs(T(v), T(joints), T(weights), T(mats)).cpu().numpy()
    assert np.array_equal(bits(out), bits(skin.skin_lbs_host(v, joints, weights, mats)))


# ------------------------------------------------------------------------------------------------ the binding
def test_a_library_without_the_entries_names_the_rebuild():
    """load_skin on a library object that lacks the new symbols raises the usual message; load() and load_all() do not
    look at them."""
    from humannerf_amd import _lib

    class Fn:
        restype = argtypes = None
    sigs = _lib.SKIN_SIGNATURES
    assert set(sigs) == {'hnrf_skin_weights', 'hnrf_skin_lbs'} and not set(sigs) & set(_lib.SIGNATURES)
    assert 'skin' not in _lib.GROUPS and list(_lib.LATE_GROUPS) == ['skin']
    old = type('OldLib', (), {})()
    with pytest.raises(_lib.HnrfError) as e:
        _lib.load_skin(old)
    assert str(e.value) == ('%s does not export %s: it was built before the skinned glTF export (include/hnrf_skin.h); '
                            'rebuild it' % (_lib.LIB_PATH, next(iter(sigs))))
    lib = _lib.load_all()
    assert lib is _lib.load() and _lib.load_late() is lib and _lib.load_skin() is lib
    whole = type('NewLib', (), {name: Fn() for name in sigs})()
    assert _lib.load_skin(whole) is whole
    assert all((getattr(whole, n).restype, getattr(whole, n).argtypes) == sigs[n] for n in sigs)


# ------------------------------------------------------------------------------------------------ end to end
LEVEL = 10.0           # with the sigma bias raised by 5 (with_density), as tests/test_gpu_mesh.py cuts the surface


@pytest.fixture(scope='module')
def net():
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state, with_density
    state = with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0)
    n = Network()
    n.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return n.to(dev()).eval()


@pytest.fixture(scope='module')
def subject(tmp_path_factory):
    from humannerf_amd import dataset, scene
    root = str(tmp_path_factory.mktemp('subject'))
    scene.write_synthetic_subject(root, n_frames=3, size=64)
    return dataset.Subject(root)


@pytest.fixture
def kick_in():
    """The pose refiner's kick-in as the reference's ZJU-MoCap configurations set it (the package's default has none:
    the refiner always acts)."""
    from humannerf_amd.config import cfg
    cfg.pose_decoder.kick_in_iter = 20000
    yield 20000
    cfg.pose_decoder.pop('kick_in_iter', None)


def projected_joint_matrices(net, frame, iter_val):
    """The joint matrices of a frame in fp64 (J, 3, 4) from rotations a quaternion can hold: dst_Rs with the refiner
    applied as include/hnrf.h states it, each projected onto the nearest rotation, chained along the SMPL tree and
    multiplied by cnl_gtfms^-1 -- restated here, not taken from the file.  Also returns the same from the unprojected
    rotations (what Network.frame_motion inverts)."""
    from humannerf_amd import gltf, scene
    rvec = net.refiner_rvec(frame, iter_val)
    R = gltf.refined_rotations(frame['dst_Rs'], None if rvec is None else rvec.cpu().numpy())
    out = []
    for rot in (gltf.nearest_rotation(R), R):
        G = np.tile(np.eye(4), (24, 1, 1))
        G[:, :3, :3], G[:, :3, 3] = rot, frame['dst_Ts'].astype(np.float64)
        A = [G[0]]
        for i in range(1, 24):
            A.append(A[scene.SMPL_PARENT[i]] @ G[i])
        inv = np.linalg.inv(frame['cnl_gtfms'].astype(np.float64))
        out.append(np.stack([(A[i] @ inv[i])[:3] for i in range(24)]))
    return out


@pytest.mark.parametrize('influences,iter_val,refines', [(4, 1e7, True), (8, 0.0, False)],
                         ids=['K4-refiner-on', 'K8-refiner-off'])
def test_run_gltf_end_to_end(net, subject, tmp_path, kick_in, influences, iter_val, refines):
    """run.run_gltf on a seeded network and a synthetic subject of 3 frames at resolution 32.  The file, read by the
    walker and re-posed in fp64, against fp64 skinning of the same truncated weights with joint matrices restated here
    from PROJECTED rotations (a quaternion holds nothing else); the floor of the _check rule is hnrf_skin_lbs itself,
    run on those matrices.  The returned skin_error and kept against the same device calls made here (equal: the
    kernels are deterministic).  The distance between projected and unprojected matrices is printed: the theta + 1e-5
    artefact of scene.rodrigues, which skin_error (defined on Network.frame_motion) does not contain."""
    from humannerf_amd import run
    assert net._refines_pose(iter_val) == refines
    res = run.run_gltf(net, subject, resolution=32, level=LEVEL, influences=influences, fps=30, logdir=str(tmp_path),
                       iter_val=iter_val)
    assert res['path'].endswith('mesh/avatar.glb') and res['frames'] == [0, 1, 2]
    doc, arr = walker.walk(res['path'])
    at = walker.attributes(doc, arr)
    assert res['V'] == len(at['POSITION']) > 100 and res['F'] * 3 == len(at['indices']) > 300
    assert at['joints'].shape == (res['V'], influences)
    verts = T(at['POSITION'])
    joints, weights, kept = net.skin_weights(verts, subject.movement_frame(0, image_size=(1, 1)), k=influences)
    assert np.array_equal(joints.cpu().numpy(), at['joints']) and np.array_equal(bits(weights.cpu().numpy()), bits(at['weights']))
    assert res['kept'] == {'min': float(kept.min()), 'mean': float(kept.mean())} and 0 < res['kept']['min'] <= res['kept']['mean'] <= 1
    srefs.check_rows(at['joints'], at['weights'], kept.cpu().numpy())
    x64 = np.concatenate([at['POSITION'].astype(np.float64), np.ones((res['V'], 1))], 1)
    per_frame = []
    for i in range(3):
        frame = subject.movement_frame(i, image_size=(1, 1))
        proj, raw = projected_joint_matrices(net, frame, iter_val)
        r64 = np.zeros((res['V'], 3))
        for k in range(influences):
            r64 += at['weights'][:, k, None].astype(np.float64) * np.einsum('vij,vj->vi', proj[at['joints'][:, k]], x64)
        r32 = skin.skin_lbs(verts, joints, weights, T(proj.astype(np.float32))).cpu()
        print('RATIO gltf K%d frame %d: projected vs unprojected joint matrices %.3e' % (influences, i, np.abs(proj - raw).max()))
        _check('gltf K%d frame %d file vs skin_lbs' % (influences, i), walker.posed(doc, arr, i), torch.from_numpy(r64), r32)
        # the returned error: |skin_lbs of frame_motion's matrices - pose_vertices|, per vertex in metres
        Rs, Ts, _ = net.frame_motion(frame, iter_val)
        assert float(np.abs(skin.joint_matrices(Rs, Ts).cpu().numpy() - raw).max()) <= 1e-5
        d = skin.skin_lbs(verts, joints, weights, skin.joint_matrices(Rs, Ts)) - net.pose_vertices(verts, frame, iter_val)
        d = torch.sqrt((d * d).sum(1))
        per_frame.append({'max': float(d.max()), 'mean': float(d.mean())})
    assert res['skin_error']['per_frame'] == per_frame
    assert res['skin_error']['max'] == max(p['max'] for p in per_frame)
    assert abs(res['skin_error']['mean'] - np.mean([p['mean'] for p in per_frame])) <= 1e-12
    assert 0 < res['skin_error']['mean'] <= res['skin_error']['max'] < 1.0
    print('RATIO gltf K%d skin_error max %.3e mean %.3e kept min %.3f mean %.3f bytes %d' % (
        influences, res['skin_error']['max'], res['skin_error']['mean'], res['kept']['min'], res['kept']['mean'],
        len(open(res['path'], 'rb').read())))


def test_refiner_changes_the_animation(net, subject, tmp_path, kick_in):
    """The two settings of the end-to-end test do differ: with the refiner on, the joints' quaternions move."""
    from humannerf_amd import run
    files = [run.run_gltf(net, subject, frames=[1], resolution=32, level=LEVEL, logdir=str(tmp_path / tag), iter_val=it)['path']
             for tag, it in (('on', 1e7), ('off', 0.0))]
    (doc_a, arr_a), (doc_b, arr_b) = (walker.walk(f) for f in files)
    rot = lambda doc, arr: np.stack([arr[doc['animations'][0]['samplers'][c['sampler']]['output']][0]
                                     for c in doc['animations'][0]['channels'] if c['target']['path'] == 'rotation'])
    qa, qb = rot(doc_a, arr_a), rot(doc_b, arr_b)
    assert np.array_equal(qa[:2], qb[:2]) and np.abs(qa[2:] - qb[2:]).max() > 1e-4       # (global and the root joint: not refined)
