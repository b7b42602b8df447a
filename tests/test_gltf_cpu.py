"""humannerf_amd/gltf.py without a GPU: the .glb container, accessors, skeleton, skin and animation of write_glb read by
an independent walker (tests/gltf_walker.py), read_glb / pose against that walker, and the kinematics: the joint
matrices a viewer forms from the file against the fp64 inverse of the motion basis, restated here from the formula of
include/hnrf.h (hnrf_motion_basis_fwd).  Tolerances: the rule of tests/test_gpu_mesh_kernels.py::_check."""
import json

import numpy as np
import pytest
import torch

from humannerf_amd import gltf, mesh, scene, skin
from tests import gltf_walker as walker
from tests.test_gpu_mesh_kernels import _check

J = 24
PARENT = scene.SMPL_PARENT
T_FRAMES = 5
MOVING_JOINT = 7


def unit_quaternions(rs, n):
    q = rs.randn(n, 4)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def quat_matrix(q):
    """Rotation matrices of unit quaternions (x, y, z, w), fp64 (the textbook form, written here on its own)."""
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def avatar(K, kind, seed=0):
    """A small avatar on the synthetic T-pose skeleton: 300 vertices in the canonical bbox, weights from the twin of
    hnrf_skin_weights on a random softmax volume, and T_FRAMES frames.  kind 'exact': dst_Rs from unit quaternions;
    'rodrigues': scene.body_pose_to_body_RTs poses (not exactly orthonormal).  One joint's dst_Ts varies."""
    rs = np.random.RandomState(seed)
    joints3d = scene.TPOSE_JOINTS
    mn, mx = joints3d.min(0) - 0.3, joints3d.max(0) + 0.3
    verts = (mn + rs.uniform(0.02, 0.98, (300, 3)) * (mx - mn)).astype(np.float32)
    faces = rs.randint(0, 300, (500, 3)).astype(np.int32)
    colors = rs.uniform(0, 1, (300, 3)).astype(np.float32)
    gen = torch.Generator().manual_seed(seed)
    vol = torch.softmax(torch.randn(J + 1, 8, 8, 8, generator=gen, dtype=torch.float64) * 3.0, 0).numpy().astype(np.float32)
    jn, wt, kept = skin.skin_weights_host(verts, vol, mn.astype(np.float32), (2.0 / (mx - mn)).astype(np.float32), k=K)
    cnl = scene.get_canonical_global_tfms(joints3d)
    Rs, Ts = [], []
    for t in range(T_FRAMES):
        if kind == 'exact':
            R = quat_matrix(unit_quaternions(rs, J)).astype(np.float32)
            _, T = scene.body_pose_to_body_RTs(np.zeros(72), joints3d)
        else:
            R, T = scene.body_pose_to_body_RTs(rs.randn(72) * 0.5, joints3d)
        T = T.copy()
        T[MOVING_JOINT] += np.float32(0.01 * t)
        Rs.append(R), Ts.append(T)
    Rh = rs.randn(T_FRAMES, 3) * 0.7
    Th = rs.uniform(-1, 1, (T_FRAMES, 3)).astype(np.float32)
    return dict(verts=verts, faces=faces, colors=colors, joints=jn, weights=wt, kept=kept, cnl_gtfms=cnl,
                dst_Rs=np.stack(Rs), dst_Ts=np.stack(Ts), Rh=Rh, Th=Th)


def write(av, path, **kw):
    return gltf.write_glb(str(path), av['verts'], av['faces'], av['colors'], av['joints'], av['weights'], av['cnl_gtfms'],
                          dst_Rs=av['dst_Rs'], dst_Ts=av['dst_Ts'], Rh=av['Rh'], Th=av['Th'], **kw)


def inverse_basis(dst_Rs, dst_Ts, cnl_gtfms, dtype):
    """A_i cnl_gtfms_i^-1 with A_i = A_parent(i) [R_i | T_i] along the SMPL tree -- the inverse of what
    hnrf_motion_basis_fwd returns (include/hnrf.h) -- in ``dtype``: (J, 4, 4)."""
    G = np.tile(np.eye(4, dtype=dtype), (J, 1, 1))
    G[:, :3, :3], G[:, :3, 3] = dst_Rs.astype(dtype), dst_Ts.astype(dtype)
    A = [G[0]]
    for i in range(1, J):
        A.append((A[PARENT[i]] @ G[i]).astype(dtype))
    inv = np.linalg.inv(cnl_gtfms.astype(np.float64)).astype(dtype)          # (pure translations: exact)
    return np.stack([(A[i] @ inv[i]).astype(dtype) for i in range(J)])


# ------------------------------------------------------------------------------------------------ the writer
@pytest.mark.parametrize('K', [4, 8])
def test_file_structure(tmp_path, K):
    av = avatar(K, 'rodrigues')
    total = write(av, tmp_path / 'a.glb', fps=25)
    doc, arr = walker.walk(str(tmp_path / 'a.glb'))              # container, chunk padding, views, alignment, min / max
    assert total == (tmp_path / 'a.glb').stat().st_size
    assert doc['asset']['version'] == '2.0' and doc['extensionsUsed'] == ['KHR_materials_unlit']
    mat = doc['materials'][0]
    assert 'KHR_materials_unlit' in mat['extensions'] and mat['pbrMetallicRoughness']['baseColorFactor'] == [1.0] * 4
    prim = doc['meshes'][0]['primitives'][0]
    assert set(prim['attributes']) == {'POSITION', 'COLOR_0'} | {'%s_%d' % (n, s) for n in ('JOINTS', 'WEIGHTS')
                                                                 for s in range(K // 4)}
    acc = lambda name: doc['accessors'][prim['attributes'][name]]
    assert (acc('POSITION')['componentType'], acc('POSITION')['type']) == (5126, 'VEC3') and 'min' in acc('POSITION')
    assert (acc('COLOR_0')['componentType'], acc('COLOR_0')['type'], acc('COLOR_0')['normalized']) == (5121, 'VEC4', True)
    assert (acc('JOINTS_0')['componentType'], acc('JOINTS_0')['type']) == (5121, 'VEC4')
    assert (acc('WEIGHTS_0')['componentType'], acc('WEIGHTS_0')['type']) == (5126, 'VEC4')
    assert doc['accessors'][prim['indices']]['componentType'] == 5125
    at = walker.attributes(doc, arr)
    assert np.array_equal(at['POSITION'], av['verts']) and np.array_equal(at['indices'], av['faces'].reshape(-1))
    assert np.array_equal(at['COLOR_0'][:, :3], mesh._u8_colors(av['colors'])) and (at['COLOR_0'][:, 3] == 255).all()
    assert np.array_equal(at['joints'], av['joints']) and np.array_equal(at['weights'].view(np.uint32), av['weights'].view(np.uint32))
    # weights: non-negative, rows summing to 1 within 4 ulp, no joint twice with a non-zero weight
    w = at['weights'].astype(np.float64)
    assert (w >= 0).all() and np.abs(w.sum(1) - 1).max() <= 4 * 2.0 ** -23
    for jr, wr in zip(at['joints'], at['weights']):
        live = jr[wr > 0].tolist()
        assert len(live) == len(set(live)) and max(live) < J
    # nodes: root > global > joint_00 .. joint_23 along the SMPL tree; the mesh node at the scene root
    names = [n.get('name') for n in doc['nodes']]
    assert names[:2] == ['root', 'global'] and names[2:2 + J] == ['joint_%02d' % i for i in range(J)]
    mesh_node = [k for k, n in enumerate(doc['nodes']) if 'mesh' in n][0]
    assert doc['scenes'][0]['nodes'] == [0, mesh_node] and doc['nodes'][mesh_node]['skin'] == 0
    assert doc['nodes'][0]['children'] == [1] and doc['nodes'][1]['children'] == [2]
    for i in range(J):
        kids = sorted(c - 2 for c in doc['nodes'][2 + i].get('children', []))
        assert kids == np.nonzero(PARENT == i)[0].tolist()
        assert 'rotation' not in doc['nodes'][2 + i]
    g = av['cnl_gtfms'].astype(np.float64)
    rest = np.array([doc['nodes'][2 + i]['translation'] for i in range(J)])
    want = g[:, :3, 3].copy()
    want[1:] -= g[PARENT[1:], :3, 3]
    assert np.array_equal(rest.astype(np.float32), want.astype(np.float32))
    sk = doc['skins'][0]
    assert sk['joints'] == list(range(2, 2 + J)) and sk['skeleton'] == 2
    ibm = arr[sk['inverseBindMatrices']].reshape(J, 4, 4).transpose(0, 2, 1)
    assert doc['accessors'][sk['inverseBindMatrices']]['type'] == 'MAT4'
    assert np.array_equal(ibm, np.linalg.inv(g).astype(np.float32))
    # without the animation: the canonical pose
    assert np.abs(walker.posed(doc, arr, None) - av['verts']).max() <= 1e-6
    # animation
    an = doc['animations']
    assert len(an) == 1 and all(s['interpolation'] == 'LINEAR' for s in an[0]['samplers'])
    times = arr[an[0]['samplers'][0]['input']].reshape(-1)
    assert len({s['input'] for s in an[0]['samplers']}) == 1 and 'min' in doc['accessors'][an[0]['samplers'][0]['input']]
    assert np.array_equal(times, (np.arange(T_FRAMES) / 25.0).astype(np.float32)) and (np.diff(times) > 0).all()
    targets = [(c['target']['node'], c['target']['path']) for c in an[0]['channels']]
    assert len(targets) == len(set(targets))
    assert sorted(n for n, p in targets if p == 'rotation') == list(range(1, 2 + J))
    assert sorted(n for n, p in targets if p == 'translation') == [1, 2 + MOVING_JOINT]
    for ch in an[0]['channels']:
        out = arr[an[0]['samplers'][ch['sampler']]['output']]
        assert len(out) == T_FRAMES
        if ch['target']['path'] == 'rotation':
            q = out.astype(np.float64)
            assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 1e-6
            assert ((q[1:] * q[:-1]).sum(1) >= 0).all()
    tr = {c['target']['node']: arr[an[0]['samplers'][c['sampler']]['output']] for c in an[0]['channels']
          if c['target']['path'] == 'translation'}
    assert np.array_equal(tr[1], av['Th']) and np.array_equal(tr[2 + MOVING_JOINT], av['dst_Ts'][:, MOVING_JOINT])


def test_read_glb_and_pose_agree_with_the_walker(tmp_path):
    av = avatar(8, 'rodrigues', seed=1)
    write(av, tmp_path / 'a.glb')
    doc, arr = walker.walk(str(tmp_path / 'a.glb'))
    glb = gltf.read_glb(str(tmp_path / 'a.glb'))
    assert glb['json'] == doc and len(glb['accessors']) == len(arr)
    for a, b in zip(glb['accessors'], arr):
        assert a.dtype == b.dtype and np.array_equal(a.reshape(b.shape).view(np.uint8), b.view(np.uint8))
    for i in (None, 0, T_FRAMES - 1):
        for rel in (None, 'global'):
            a, b = gltf.pose(glb, i, relative_to=rel), walker.posed(doc, arr, i, relative_to=rel)
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize('up,axis', [('+z', [0, 0, 1]), ('+y', [0, 1, 0]), ('-y', [0, -1, 0])])
def test_up_axis_and_global_transform(tmp_path, up, axis):
    """The root turns the world's up axis into glTF's +Y; ``global`` carries x_world = R(Rh) x + Th."""
    from humannerf_amd.dataset import rodrigues_cv
    av = avatar(4, 'exact', seed=2)
    write(av, tmp_path / 'a.glb', up=up)
    doc, arr = walker.walk(str(tmp_path / 'a.glb'))
    U = walker.world_matrices(doc, arr, None)[0][:3, :3]
    assert np.abs(U @ np.array(axis, float) - [0, 1, 0]).max() <= 1e-7 and abs(np.linalg.det(U) - 1) <= 1e-6
    assert 'animations' in doc and all(c['target']['node'] != 0 for c in doc['animations'][0]['channels'])
    for i in (0, 3):
        body = walker.posed(doc, arr, i, relative_to='global')
        world = walker.posed(doc, arr, i, relative_to=None)
        want = (body @ rodrigues_cv(av['Rh'][i]).T + av['Th'][i].astype(np.float64)) @ U.T
        assert np.abs(world - want).max() <= 2e-6
    with pytest.raises(ValueError):
        write(av, tmp_path / 'b.glb', up='z')


def test_no_frames_no_animation_and_bad_input(tmp_path):
    av = avatar(4, 'exact')
    gltf.write_glb(str(tmp_path / 'a.glb'), av['verts'], av['faces'], av['colors'], av['joints'], av['weights'], av['cnl_gtfms'])
    doc, arr = walker.walk(str(tmp_path / 'a.glb'))
    rest = gltf.pose(gltf.read_glb(str(tmp_path / 'a.glb')), relative_to='global')
    assert 'animations' not in doc and np.abs(rest - av['verts']).max() <= 1e-6
    with pytest.raises(ValueError):
        gltf.write_glb(str(tmp_path / 'b.glb'), av['verts'], av['faces'] + 300, av['colors'], av['joints'], av['weights'], av['cnl_gtfms'])
    with pytest.raises(ValueError):
        gltf.write_glb(str(tmp_path / 'b.glb'), av['verts'], av['faces'], av['colors'], av['joints'][:, :3], av['weights'][:, :3], av['cnl_gtfms'])
    with pytest.raises(ValueError):
        gltf.write_glb(str(tmp_path / 'b.glb'), av['verts'][:0], av['faces'][:0], av['colors'][:0], av['joints'][:0], av['weights'][:0], av['cnl_gtfms'])


# ------------------------------------------------------------------------------------------------ kinematics
def test_exact_rotations_reproduce_the_inverse_motion_basis(tmp_path):
    """dst_Rs built from unit quaternions: the joint matrices a viewer forms from the file (in the frame of ``global``)
    are the fp64 inverse of the motion basis, to the floor of its own fp32 evaluation."""
    av = avatar(4, 'exact', seed=3)
    write(av, tmp_path / 'a.glb')
    doc, arr = walker.walk(str(tmp_path / 'a.glb'))
    for i in range(T_FRAMES):
        got = walker.joint_matrices(doc, arr, i)[:, :3]
        r64 = inverse_basis(av['dst_Rs'][i], av['dst_Ts'][i], av['cnl_gtfms'], np.float64)[:, :3]
        r32 = inverse_basis(av['dst_Rs'][i], av['dst_Ts'][i], av['cnl_gtfms'], np.float32)[:, :3]
        _check('gltf exact frame %d joint matrices' % i, got, torch.from_numpy(r64), torch.from_numpy(r32))


def test_rodrigues_poses_reproduce_the_projected_reference(tmp_path):
    """scene.body_pose_to_body_RTs divides by theta + 1e-5: its matrices are not rotations, and a quaternion cannot
    hold them.  The file must match the fp64 reference built from the SVD-projected rotations; the distance of that
    reference from the unprojected one is printed -- the input's artefact, not an error of the export."""
    av = avatar(4, 'rodrigues', seed=4)
    write(av, tmp_path / 'a.glb')
    doc, arr = walker.walk(str(tmp_path / 'a.glb'))
    for i in range(T_FRAMES):
        got = walker.joint_matrices(doc, arr, i)[:, :3]
        proj = gltf.nearest_rotation(av['dst_Rs'][i])
        assert np.abs(proj @ proj.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14 and (np.linalg.det(proj) > 0).all()
        r64 = inverse_basis(proj, av['dst_Ts'][i], av['cnl_gtfms'], np.float64)[:, :3]
        r32 = inverse_basis(proj, av['dst_Ts'][i], av['cnl_gtfms'], np.float32)[:, :3]
        raw = inverse_basis(av['dst_Rs'][i], av['dst_Ts'][i], av['cnl_gtfms'], np.float64)[:, :3]
        print('RATIO gltf rodrigues frame %d: projected vs unprojected reference %.3e' % (i, np.abs(raw - r64).max()))
        _check('gltf rodrigues frame %d joint matrices' % i, got, torch.from_numpy(r64), torch.from_numpy(r32))


def test_refined_rotations_restate_the_refiner():
    """dst_Rs[i] Rodrigues(rvec[i - 1]) with theta = sqrt(1e-5 + |r|^2), against network.rodrigues in fp64."""
    from humannerf_amd.network import rodrigues
    rs = np.random.RandomState(6)
    R, _ = scene.body_pose_to_body_RTs(rs.randn(72) * 0.3, scene.TPOSE_JOINTS)
    rvec = rs.randn(J - 1, 3) * 0.05
    got = gltf.refined_rotations(R, rvec)
    want = R.astype(np.float64).copy()
    want[1:] = want[1:] @ rodrigues(torch.from_numpy(rvec)).numpy()
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-15
    assert np.array_equal(gltf.refined_rotations(R, None), R.astype(np.float64))


def test_quaternions_cover_every_branch():
    rs = np.random.RandomState(7)
    q = unit_quaternions(rs, 200)
    q[:4] = np.eye(4)                                            # rotations by pi about x, y, z and the identity
    q[4:8] = np.eye(4) + 1e-9
    q[4:8] /= np.linalg.norm(q[4:8], axis=1, keepdims=True)
    back = gltf.quaternion(quat_matrix(q))
    sign = np.sign((back * q).sum(1))[:, None]
    assert np.abs(back * sign - q).max() <= 1e-12 and np.abs(np.linalg.norm(back, axis=1) - 1).max() <= 1e-15
    assert np.abs(gltf.quaternion_matrix(q) - quat_matrix(q)).max() <= 1e-15
