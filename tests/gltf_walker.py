"""A reader of .glb files for the tests of the skinned export, written from the glTF 2.0 specification and sharing no
code with humannerf_amd/gltf.py: container and accessor checks, and the pose of key-frame i in float64."""
import json
import struct

import numpy as np

COMPONENT = {5120: ('i1', 1), 5121: ('u1', 1), 5122: ('<i2', 2), 5123: ('<u2', 2), 5125: ('<u4', 4), 5126: ('<f4', 4)}
WIDTH = {'SCALAR': 1, 'VEC2': 2, 'VEC3': 3, 'VEC4': 4, 'MAT4': 16}


def walk(path):
    """Checks the container and every bufferView / accessor on the way; returns (document, [array per accessor])."""
    raw = open(path, 'rb').read()
    assert raw[:4] == b'glTF' and struct.unpack('<I', raw[4:8])[0] == 2
    assert struct.unpack('<I', raw[8:12])[0] == len(raw) and len(raw) % 4 == 0
    jlen, jtype = struct.unpack('<I4s', raw[12:20])
    assert jtype == b'JSON' and jlen % 4 == 0
    text = raw[20:20 + jlen]
    assert text.rstrip(b' ') == text.strip() and b'\0' not in text            # padded with spaces, at the end only
    doc = json.loads(text.decode('utf-8'))
    blen, btype = struct.unpack('<I4s', raw[20 + jlen:28 + jlen])
    assert btype == b'BIN\0' and blen % 4 == 0 and 28 + jlen + blen == len(raw)
    blob = raw[28 + jlen:]
    assert len(doc['buffers']) == 1 and 'uri' not in doc['buffers'][0]
    need = doc['buffers'][0]['byteLength']
    assert need <= blen < need + 4 and blob[need:] == b'\0' * (blen - need)    # padded with zeros
    for view in doc['bufferViews']:
        assert view['buffer'] == 0 and view.get('byteOffset', 0) % 4 == 0
        assert 0 <= view.get('byteOffset', 0) and view.get('byteOffset', 0) + view['byteLength'] <= need
        assert view.get('byteStride', 4) % 4 == 0
    arrays = []
    for acc in doc['accessors']:
        code, size = COMPONENT[acc['componentType']]
        view, n = doc['bufferViews'][acc['bufferView']], WIDTH[acc['type']]
        off = acc.get('byteOffset', 0)
        assert off % size == 0 and (view.get('byteOffset', 0) + off) % size == 0
        stride = view.get('byteStride', n * size)
        assert stride % 4 == 0 or 'target' not in view or view['target'] == 34963    # vertex data: rows of 4 bytes
        assert off + (acc['count'] - 1) * stride + n * size <= view['byteLength'] and acc['count'] >= 1
        start = view.get('byteOffset', 0) + off
        rows = [np.frombuffer(blob, code, n, start + r * stride) for r in range(acc['count'])] if stride != n * size \
            else np.frombuffer(blob, code, n * acc['count'], start).reshape(acc['count'], n)
        arr = np.array(rows)
        if 'min' in acc:
            assert np.array_equal(np.array(acc['min'], arr.dtype), arr.min(0)) and np.array_equal(np.array(acc['max'], arr.dtype), arr.max(0))
        arrays.append(arr)
    return doc, arrays


def _rot(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def world_matrices(doc, arrays, i):
    """Global 4x4 of every node at key-frame i (None: as the nodes stand)."""
    trs = [{'translation': n.get('translation', [0, 0, 0]), 'rotation': n.get('rotation', [0, 0, 0, 1]),
            'scale': n.get('scale', [1, 1, 1])} for n in doc['nodes']]
    if i is not None:
        anim = doc['animations'][0]
        for ch in anim['channels']:
            trs[ch['target']['node']][ch['target']['path']] = arrays[anim['samplers'][ch['sampler']]['output']][i]
    out = {}

    def down(n, parent):
        local = np.eye(4)
        local[:3, :3] = _rot(trs[n]['rotation']) @ np.diag(np.asarray(trs[n]['scale'], float))
        local[:3, 3] = np.asarray(trs[n]['translation'], float)
        out[n] = parent @ local
        for c in doc['nodes'][n].get('children', []):
            down(c, out[n])
    for n in doc['scenes'][doc['scene']]['nodes']:
        down(n, np.eye(4))
    return out


def node_named(doc, name):
    return [k for k, n in enumerate(doc['nodes']) if n.get('name') == name][0]


def joint_matrices(doc, arrays, i, relative_to='global'):
    """(J, 4, 4) float64: world(joint) x inverseBind, in the frame of node ``relative_to`` (None: the world)."""
    skin = doc['skins'][0]
    world = world_matrices(doc, arrays, i)
    ibm = arrays[skin['inverseBindMatrices']].astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)     # column-major
    base = np.eye(4) if relative_to is None else np.linalg.inv(world[node_named(doc, relative_to)])
    return np.stack([base @ world[j] @ ibm[k] for k, j in enumerate(skin['joints'])])


def attributes(doc, arrays):
    """POSITION (V, 3), COLOR_0 (V, 4), joints (V, K), weights (V, K) and the indices of the one primitive."""
    prim = doc['meshes'][0]['primitives'][0]
    at = prim['attributes']
    sets = sorted(int(k.split('_')[1]) for k in at if k.startswith('JOINTS_'))
    assert sets == list(range(len(sets))) and all('WEIGHTS_%d' % s in at for s in sets)
    return {'POSITION': arrays[at['POSITION']], 'COLOR_0': arrays[at['COLOR_0']],
            'joints': np.concatenate([arrays[at['JOINTS_%d' % s]] for s in sets], 1),
            'weights': np.concatenate([arrays[at['WEIGHTS_%d' % s]] for s in sets], 1),
            'indices': arrays[prim['indices']].reshape(-1)}


def posed(doc, arrays, i, relative_to='global'):
    """The skinned vertices (V, 3) of key-frame i in float64."""
    at, jm = attributes(doc, arrays), joint_matrices(doc, arrays, i, relative_to)
    x = np.concatenate([at['POSITION'].astype(np.float64), np.ones((len(at['POSITION']), 1))], 1)
    out = np.zeros((len(x), 3))
    for k in range(at['joints'].shape[1]):
        out += at['weights'][:, k, None].astype(np.float64) * np.einsum('vij,vj->vi', jm[at['joints'][:, k]][:, :3], x)
    return out
