"""The avatar as one skinned, animated glTF 2.0 binary (.glb), written with ``json`` and ``struct`` alone.

The forward skinning of this package is, term for term, what glTF calls skinning::

    x_o = sum_b  w_b(x_c) / max(sum w, 1e-4) . (A_b . cnl_gtfms_b^-1) x_c
          `-- WEIGHTS_n / JOINTS_n ---------'   |     `-- inverseBindMatrices[b]
                                                `-- world transform of joint node b (SMPL tree, local R_b | T_b)

so the file holds the canonical mesh and its vertex colours once, a 24-joint skeleton, per-vertex weights (the K
largest of skin.skin_weights, K = 4 or 8) and one animation with a quaternion per joint per frame.  What it does NOT
hold: the non-rigid offsets (skinning cannot represent them; the export is the geometry class of run.run_mesh and the
mesh preview), the weights beyond the K largest (run.run_gltf measures what that costs), textures, cameras.  Normals
are optional (``write_glb(normals=...)``: the density-gradient normals of Network.vertex_normals, bind pose); without
them a viewer shades every face flat.

Layout of the file (``write_glb``):

- container: 12-byte header, a JSON chunk padded with spaces and a BIN chunk padded with zeros, each to 4 bytes;
- one buffer; indices UNSIGNED_INT; POSITION VEC3 FLOAT with min / max; COLOR_0 VEC4 UNSIGNED_BYTE normalised, alpha
  255, quantised like mesh.write_ply; JOINTS_0 VEC4 UNSIGNED_BYTE, WEIGHTS_0 VEC4 FLOAT (JOINTS_1 / WEIGHTS_1 when
  K = 8); with normals NORMAL VEC3 FLOAT behind them; every bufferView starts on a multiple of 4 and is tightly packed;
- material: KHR_materials_unlit, white -- the vertex colours are radiance the network already shaded;
- nodes: ``root`` (static: the up-axis rotation into glTF's +Y-up world) > ``global`` (the frame's Rh / Th: x_world =
  R(Rh) x + Th) > ``joint_00`` .. ``joint_23`` along scene.SMPL_PARENT, rest translation = the canonical
  parent-relative offset, rest rotation identity: without the animation a viewer shows the canonical pose.  The mesh
  node (mesh + skin) sits at the scene root;
- skin: the 24 joints, inverseBindMatrices = cnl_gtfms^-1 (MAT4 FLOAT, column-major), skeleton = joint_00;
- animation: LINEAR samplers over t_i = i / fps; a rotation channel per joint and for ``global``, a translation
  channel for ``global``, and one for a joint only where its dst_Ts differs from the rest translation in some frame
  (so also where it varies).  Every rotation is projected onto the nearest rotation matrix (SVD, float64) before it
  becomes a unit quaternion -- scene.rodrigues divides by theta + 1e-5, its matrices are not exactly orthonormal --
  and dot(q_t, q_{t-1}) >= 0 per node.

``read_glb`` reads such a file back (JSON plus one array per accessor) and ``pose`` evaluates key-frame i by the letter
of the specification, in float64, from the file alone: a way to check a file without a viewer.  No glTF viewer or
validator has seen these files (none is available where this was written).
"""
import json
import struct

import numpy as np

from .scene import SMPL_PARENT

GLB_MAGIC, GLB_VERSION, CHUNK_JSON, CHUNK_BIN = 0x46546C67, 2, 0x4E4F534A, 0x004E4942
BYTE, UBYTE, SHORT, USHORT, UINT, FLOAT = 5120, 5121, 5122, 5123, 5125, 5126
ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 34962, 34963
_DTYPES = {BYTE: 'i1', UBYTE: 'u1', SHORT: '<i2', USHORT: '<u2', UINT: '<u4', FLOAT: '<f4'}
_NCOMP = {'SCALAR': 1, 'VEC2': 2, 'VEC3': 3, 'VEC4': 4, 'MAT2': 4, 'MAT3': 9, 'MAT4': 16}

# body-world axes -> glTF's right-handed +Y-up world, as rotation matrices (x_gltf = U x_world)
UP = {'+y': np.eye(3),
      '+z': np.array([[1.0, 0, 0], [0, 0, 1], [0, -1, 0]]),           # ZJU-MoCap: the orbit of dataset.ROT_CAM_PARAMS turns about z
      '-y': np.array([[1.0, 0, 0], [0, -1, 0], [0, 0, -1]])}          # a camera-convention world (y down)


# ------------------------------------------------------------------------------------------------------ rotations
def nearest_rotation(M):
    """The rotation matrix nearest to every 3x3 of M (..., 3, 3) in the Frobenius norm: U diag(1, 1, det(U V^T)) V^T of
    the SVD, float64."""
    M = np.asarray(M, dtype=np.float64)
    U, _, Vt = np.linalg.svd(M)
    d = np.linalg.det(U @ Vt)
    D = np.zeros(M.shape)
    D[..., 0, 0] = D[..., 1, 1] = 1.0
    D[..., 2, 2] = d
    return U @ D @ Vt


def quaternion(R):
    """Unit quaternions (..., 4) as glTF orders them, (x, y, z, w), of rotation matrices (..., 3, 3), float64: the branch
    with the largest of w^2, x^2, y^2, z^2 (no division by a small number)."""
    R = np.asarray(R, dtype=np.float64)
    flat = R.reshape(-1, 3, 3)
    out = np.empty((len(flat), 4))
    for n, m in enumerate(flat):
        t = np.array([m[0, 0] + m[1, 1] + m[2, 2], m[0, 0] - m[1, 1] - m[2, 2], -m[0, 0] + m[1, 1] - m[2, 2],
                      -m[0, 0] - m[1, 1] + m[2, 2]])
        k = int(np.argmax(t))
        s = 2.0 * np.sqrt(max(1.0 + t[k], 0.0))
        if k == 0:
            q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
        elif k == 1:
            q = [0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s]
        elif k == 2:
            q = [(m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s]
        else:
            q = [(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s, (m[1, 0] - m[0, 1]) / s]
        q = np.array(q)
        out[n] = q / np.linalg.norm(q)
    return out.reshape(R.shape[:-2] + (4,))


def quaternion_matrix(q):
    """Rotation matrices (..., 3, 3) of quaternions (x, y, z, w) (..., 4), float64, as the specification converts them
    (the quaternion taken as it stands)."""
    q = np.asarray(q, dtype=np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return R


def refined_rotations(dst_Rs, rvec=None):
    """The frame's local rotations (J, 3, 3) in float64 with the pose refiner applied as hnrf_refined_motion_basis_fwd
    applies it (include/hnrf.h): dst_Rs[i] <- dst_Rs[i] Rodrigues(rvec[i - 1]) for the non-root joints, theta =
    sqrt(1e-5 + |r|^2).  ``rvec`` (J - 1, 3) or None."""
    R = np.array(dst_Rs, dtype=np.float64)
    if rvec is None:
        return R
    r = np.asarray(rvec, dtype=np.float64).reshape(-1, 3)
    theta = np.sqrt(1e-5 + np.sum(r * r, axis=1))
    a = r / theta[:, None]
    c, s = np.cos(theta), np.sin(theta)
    x, y, z, oc = a[:, 0], a[:, 1], a[:, 2], 1.0 - c
    D = np.stack([x * x + (1 - x * x) * c, x * y * oc - z * s, x * z * oc + y * s,
                  x * y * oc + z * s, y * y + (1 - y * y) * c, y * z * oc - x * s,
                  x * z * oc - y * s, y * z * oc + x * s, z * z + (1 - z * z) * c], axis=1).reshape(-1, 3, 3)
    R[1:] = R[1:] @ D
    return R


def _continuous(q):
    """Flip signs along axis 0 so that dot(q_t, q_{t-1}) >= 0."""
    q = np.array(q, dtype=np.float64)
    for t in range(1, len(q)):
        flip = np.sum(q[t] * q[t - 1], axis=-1) < 0
        q[t][flip] = -q[t][flip]
    return q


# ------------------------------------------------------------------------------------------------------ writer
class _Buffer:
    def __init__(self):
        self.blob, self.views, self.accessors = bytearray(), [], []

    def view(self, data, target=None):
        assert len(self.blob) % 4 == 0
        v = {'buffer': 0, 'byteOffset': len(self.blob), 'byteLength': len(data)}
        if target is not None:
            v['target'] = target
        self.blob += data
        self.blob += b'\0' * (-len(self.blob) % 4)
        self.views.append(v)
        return len(self.views) - 1

    def accessor(self, arr, ctype, kind, target=None, minmax=False, normalized=False, view=None, offset=0):
        arr = np.ascontiguousarray(arr, dtype=_DTYPES[ctype])
        n = arr.size // _NCOMP[kind]
        assert arr.size == n * _NCOMP[kind] and offset % arr.dtype.itemsize == 0
        a = {'bufferView': self.view(arr.tobytes(), target) if view is None else view, 'componentType': ctype,
             'count': n, 'type': kind}
        if offset:
            a['byteOffset'] = offset
        if normalized:
            a['normalized'] = True
        if minmax:
            flat = arr.reshape(n, _NCOMP[kind])
            a['min'], a['max'] = [float(v) for v in flat.min(0)], [float(v) for v in flat.max(0)]
        self.accessors.append(a)
        return len(self.accessors) - 1


def _np(a, dtype):
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=dtype)


def write_glb(path, verts, faces, colors, joints, weights, cnl_gtfms, dst_Rs=None, dst_Ts=None, Rh=None, Th=None,
              fps=30, up='+z', parent=SMPL_PARENT, name='avatar', normals=None):
    """Write the skinned, animated avatar (layout: the module's docstring).

    verts (V, 3) canonical; faces (F, 3); colors (V, 3) in [0, 1] or uint8; joints (V, K) uint8 and weights (V, K),
    K = 4 or 8 (skin.skin_weights); cnl_gtfms (J, 4, 4), the canonical global transforms (pure translations).
    Animation of T frames (dst_Rs None or T = 0: none is written): dst_Rs (T, J, 3, 3) the local rotations, the pose
    refiner already applied where it acts (refined_rotations); dst_Ts (T, J, 3); Rh (T, 3) axis-angle and Th (T, 3) of
    the ``global`` node (None: identity / zero).  ``normals`` (V, 3): unit vectors in the bind pose, written as the
    NORMAL attribute behind the weights (a zero vector, where the field has no gradient, stays zero); None: the file is
    what it is without the argument, byte for byte.  Returns the number of bytes written."""
    from .dataset import rodrigues_cv
    from .mesh import _u8_colors
    if up not in UP:
        raise ValueError("up must be one of '+z', '+y', '-y'")
    v = np.ascontiguousarray(_np(verts, np.float32)).reshape(-1, 3)
    f = _np(faces, np.int64).reshape(-1, 3)
    V = len(v)
    if V == 0 or len(f) == 0:
        raise ValueError('write_glb: an empty mesh (a glTF accessor holds at least one element)')
    if f.min() < 0 or f.max() >= V:
        raise ValueError('write_glb: a face index outside [0, %d)' % V)
    jn, wt = _np(joints, np.uint8).reshape(V, -1), _np(weights, np.float32).reshape(V, -1)
    K = jn.shape[1]
    if K not in (4, 8) or wt.shape[1] != K:
        raise ValueError('write_glb: joints and weights must be (V, 4) or (V, 8)')
    g = _np(cnl_gtfms, np.float64)
    J = len(g)
    parent = np.asarray(parent, dtype=np.int64)
    if g.shape != (J, 4, 4) or len(parent) != J or parent[0] != -1 or jn.max() >= J:
        raise ValueError('write_glb: cnl_gtfms (J, 4, 4), parent (J,) with the root first, joints < J expected')
    col = _u8_colors(_np(colors, None)).reshape(V, 3)
    rgba = np.concatenate([col, np.full((V, 1), 255, np.uint8)], axis=1)

    buf = _Buffer()
    prim = {'attributes': {}, 'mode': 4, 'material': 0}
    prim['indices'] = buf.accessor(f.astype(np.uint32), UINT, 'SCALAR', ELEMENT_ARRAY_BUFFER)
    prim['attributes']['POSITION'] = buf.accessor(v, FLOAT, 'VEC3', ARRAY_BUFFER, minmax=True)
    prim['attributes']['COLOR_0'] = buf.accessor(rgba, UBYTE, 'VEC4', ARRAY_BUFFER, normalized=True)
    for s in range(K // 4):
        prim['attributes']['JOINTS_%d' % s] = buf.accessor(jn[:, 4 * s:4 * s + 4], UBYTE, 'VEC4', ARRAY_BUFFER)
        prim['attributes']['WEIGHTS_%d' % s] = buf.accessor(wt[:, 4 * s:4 * s + 4], FLOAT, 'VEC4', ARRAY_BUFFER)
    if normals is not None:
        nrm = np.ascontiguousarray(_np(normals, np.float32)).reshape(-1, 3)
        if nrm.shape[0] != V or not np.isfinite(nrm).all():
            raise ValueError('write_glb: normals must be (V, 3) and finite')
        prim['attributes']['NORMAL'] = buf.accessor(nrm, FLOAT, 'VEC3', ARRAY_BUFFER)

    # nodes: 0 root, 1 global, 2 .. J + 1 the joints, J + 2 the mesh
    ROOT, GLOBAL, JOINT0, MESH = 0, 1, 2, J + 2
    rest = g[:, :3, 3].copy()
    rest[1:] = g[1:, :3, 3] - g[parent[1:], :3, 3]
    rest = rest.astype(np.float32)
    nodes = [{'name': 'root', 'children': [GLOBAL], 'rotation': [float(x) for x in quaternion(UP[up]).astype(np.float32)]},
             {'name': 'global', 'children': [JOINT0]}]
    for i in range(J):
        n = {'name': 'joint_%02d' % i, 'translation': [float(x) for x in rest[i]]}
        kids = [JOINT0 + int(c) for c in np.nonzero(parent == i)[0]]
        if kids:
            n['children'] = kids
        nodes.append(n)
    nodes.append({'name': name, 'mesh': 0, 'skin': 0})
    ibm = np.linalg.inv(g).astype(np.float32)
    skin = {'joints': list(range(JOINT0, JOINT0 + J)), 'skeleton': JOINT0,
            'inverseBindMatrices': buf.accessor(ibm.transpose(0, 2, 1), FLOAT, 'MAT4')}       # column-major

    doc = {'asset': {'version': '2.0', 'generator': 'humannerf_amd.gltf'},
           'extensionsUsed': ['KHR_materials_unlit'],
           'scene': 0, 'scenes': [{'nodes': [ROOT, MESH]}], 'nodes': nodes,
           'meshes': [{'name': name, 'primitives': [prim]}],
           'materials': [{'name': 'radiance', 'extensions': {'KHR_materials_unlit': {}},
                          'pbrMetallicRoughness': {'baseColorFactor': [1.0, 1.0, 1.0, 1.0], 'metallicFactor': 0.0,
                                                   'roughnessFactor': 1.0}}],
           'skins': [skin]}

    T = 0 if dst_Rs is None else len(dst_Rs)
    if T:
        Rl = nearest_rotation(_np(dst_Rs, np.float64).reshape(T, J, 3, 3))
        Tl = _np(dst_Ts, np.float32).reshape(T, J, 3)
        Rg = np.stack([rodrigues_cv(r) for r in _np(Rh, np.float64).reshape(T, 3)]) if Rh is not None \
            else np.tile(np.eye(3), (T, 1, 1))
        Tg = _np(Th, np.float32).reshape(T, 3) if Th is not None else np.zeros((T, 3), np.float32)
        # (T, J + 1, 4): the global node first
        q = _continuous(quaternion(np.concatenate([nearest_rotation(Rg)[:, None], Rl], axis=1))).astype(np.float32)
        moving = [i for i in range(J) if np.any(Tl[:, i] != rest[i][None])]
        times = buf.accessor(np.arange(T, dtype=np.float64) / float(fps), FLOAT, 'SCALAR', minmax=True)
        rot_view = buf.view(np.ascontiguousarray(q.transpose(1, 0, 2)).tobytes())             # node-major
        tr = np.stack([Tg] + [Tl[:, i] for i in moving])                                      # (1 + moving, T, 3)
        tr_view = buf.view(np.ascontiguousarray(tr, dtype='<f4').tobytes())
        samplers, channels = [], []

        def channel(node, path, accessor):
            samplers.append({'input': times, 'output': accessor, 'interpolation': 'LINEAR'})
            channels.append({'sampler': len(samplers) - 1, 'target': {'node': node, 'path': path}})
        for n in range(J + 1):
            channel(GLOBAL + n, 'rotation', buf.accessor(q[:, n], FLOAT, 'VEC4', view=rot_view, offset=n * T * 16))
        for m, node in enumerate([GLOBAL] + [JOINT0 + i for i in moving]):
            channel(node, 'translation', buf.accessor(tr[m], FLOAT, 'VEC3', view=tr_view, offset=m * T * 12))
        doc['animations'] = [{'name': 'movement', 'samplers': samplers, 'channels': channels}]

    doc['accessors'], doc['bufferViews'] = buf.accessors, buf.views
    doc['buffers'] = [{'byteLength': len(buf.blob)}]
    text = json.dumps(doc, separators=(',', ':')).encode('utf-8')
    text += b' ' * (-len(text) % 4)
    blob = bytes(buf.blob) + b'\0' * (-len(buf.blob) % 4)
    total = 12 + 8 + len(text) + 8 + len(blob)
    with open(path, 'wb') as fh:
        fh.write(struct.pack('<III', GLB_MAGIC, GLB_VERSION, total))
        fh.write(struct.pack('<II', len(text), CHUNK_JSON))
        fh.write(text)
        fh.write(struct.pack('<II', len(blob), CHUNK_BIN))
        fh.write(blob)
    return total


# ------------------------------------------------------------------------------------------------------ reader
def read_glb(path):
    """A .glb as dict(json = the document, accessors = one numpy array per accessor, (count, components) or (count,)
    for SCALAR, in the file's component type; bin = the binary chunk)."""
    with open(path, 'rb') as fh:
        data = fh.read()
    magic, version, total = struct.unpack_from('<III', data, 0)
    if magic != GLB_MAGIC or version != GLB_VERSION or total != len(data):
        raise ValueError('%s: not a glTF 2.0 binary of its stated length' % path)
    n0, t0 = struct.unpack_from('<II', data, 12)
    if t0 != CHUNK_JSON:
        raise ValueError('%s: the first chunk is not JSON' % path)
    doc = json.loads(data[20:20 + n0].decode('utf-8'))
    blob = b''
    if 20 + n0 < total:
        n1, t1 = struct.unpack_from('<II', data, 20 + n0)
        if t1 != CHUNK_BIN:
            raise ValueError('%s: the second chunk is not BIN' % path)
        blob = data[28 + n0:28 + n0 + n1]
    arrays = []
    for a in doc.get('accessors', []):
        view = doc['bufferViews'][a['bufferView']]
        dt, nc = np.dtype(_DTYPES[a['componentType']]), _NCOMP[a['type']]
        start = view.get('byteOffset', 0) + a.get('byteOffset', 0)
        stride = view.get('byteStride', 0) or dt.itemsize * nc
        if start + (a['count'] - 1) * stride + dt.itemsize * nc > view.get('byteOffset', 0) + view['byteLength']:
            raise ValueError('%s: an accessor runs past its bufferView' % path)
        arr = np.ndarray((a['count'], nc), dtype=dt, buffer=blob, offset=start, strides=(stride, dt.itemsize)).copy()
        arrays.append(arr[:, 0] if nc == 1 else arr)
    res = {'json': doc, 'accessors': arrays, 'bin': blob}
    for m in doc.get('meshes', []):
        for p in m.get('primitives', []):
            if 'NORMAL' in p.get('attributes', {}) and 'normals' not in res:
                res['normals'] = arrays[p['attributes']['NORMAL']]          # (V, 3) float32 of the first such primitive
    return res


def _local_matrix(node, override):
    M = np.eye(4)
    if 'matrix' in node and not override:
        return np.array(node['matrix'], dtype=np.float64).reshape(4, 4).T
    t = override.get('translation', node.get('translation', [0, 0, 0]))
    r = override.get('rotation', node.get('rotation', [0, 0, 0, 1]))
    s = override.get('scale', node.get('scale', [1, 1, 1]))
    M[:3, :3] = quaternion_matrix(np.asarray(r, np.float64)) * np.asarray(s, np.float64)[None, :]
    M[:3, 3] = np.asarray(t, np.float64)
    return M


def node_world_matrices(glb, i=None, animation=0):
    """World matrix (4, 4) float64 of every node at key-frame ``i`` of ``animation`` (None: the rest pose): local
    matrix = T R S with the animated channels' outputs at index i in the place of the node's own, composed down the
    tree from the scene's roots."""
    doc, acc = glb['json'], glb['accessors']
    override = [dict() for _ in doc['nodes']]
    if i is not None:
        anim = doc['animations'][animation]
        for ch in anim['channels']:
            out = acc[anim['samplers'][ch['sampler']]['output']]
            override[ch['target']['node']][ch['target']['path']] = out[i]
    world = [None] * len(doc['nodes'])

    def walk(n, M):
        world[n] = M @ _local_matrix(doc['nodes'][n], override[n])
        for c in doc['nodes'][n].get('children', []):
            walk(c, world[n])
    for n in doc['scenes'][doc.get('scene', 0)]['nodes']:
        walk(n, np.eye(4))
    return world


def pose(glb, i=None, relative_to=None, animation=0):
    """The skinned POSITIONs (V, 3) float64 of the file's mesh at key-frame ``i`` (None: the rest pose), from the file
    alone: joint matrix = world(joint) x inverseBindMatrix, vertex = sum over JOINTS_n / WEIGHTS_n of weight x joint
    matrix x (POSITION, 1).  ``relative_to``: a node's name -- the result in that node's frame instead of the world's
    ('global': the body frame Network.pose_vertices works in)."""
    doc, acc = glb['json'], glb['accessors']
    node = next(n for n in doc['nodes'] if 'mesh' in n and 'skin' in n)
    skin, prim = doc['skins'][node['skin']], doc['meshes'][node['mesh']]['primitives'][0]
    world = node_world_matrices(glb, i, animation)
    ibm = acc[skin['inverseBindMatrices']].astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
    jm = np.stack([world[j] @ ibm[k] for k, j in enumerate(skin['joints'])])
    if relative_to is not None:
        ref = next(k for k, n in enumerate(doc['nodes']) if n.get('name') == relative_to)
        jm = np.linalg.inv(world[ref])[None] @ jm
    pos = acc[prim['attributes']['POSITION']].astype(np.float64)
    hom = np.concatenate([pos, np.ones((len(pos), 1))], axis=1)
    out = np.zeros((len(pos), 3))
    s = 0
    while 'JOINTS_%d' % s in prim['attributes']:
        jn = acc[prim['attributes']['JOINTS_%d' % s]].astype(np.int64)
        wt = acc[prim['attributes']['WEIGHTS_%d' % s]].astype(np.float64)
        for k in range(jn.shape[1]):
            out += wt[:, k, None] * np.einsum('vij,vj->vi', jm[jn[:, k]][:, :3], hom)
        s += 1
    return out
