"""Triangle meshes of the canonical body: isosurface extraction and mesh files.

``mesh_from_density`` runs marching tetrahedra on the device (hnrf_mesh_count / hnrf_mesh_emit, include/hnrf.h);
``mesh_from_density_host`` restates it in numpy with the same conventions, bit for bit, for CPU callers and tests
(the host/device idiom of ``imageproc``).  The conventions:

- lattice: ``density`` (N, N, N) indexed [z][y][x]; point (x, y, z) at ``bbox_min + (float32)i * step``,
  ``step = (bbox_max - bbox_min) / (N - 1)``, in float32, every operation rounded on its own;
- a point is inside when ``density > level``;
- every cell is cut into the six Kuhn tetrahedra around its main diagonal; every lattice point owns the lattice
  edges to its +x, +y, +z, +xy, +xz, +yz, +xyz neighbours (slots 0..6), and each of them that crosses the level
  carries one vertex at ``pa + t * (pb - pa)``, ``t = (level - da) / (db - da)``, a = the owning point;
- vertices are ordered by (point index, slot), triangles by (cell index, tetrahedron 0..5, triangle 0..1);
- triangles are wound counter-clockwise seen from outside: ``(v1 - v0) x (v2 - v0)`` points toward lower density.

The surface is watertight and edge-manifold except where it meets the lattice boundary, where it stays open.
Writers: ``write_ply`` (binary little-endian, uchar colours) and ``write_obj`` ('v x y z r g b' lines as
``render.ImageWriter.append_cnl_3d`` writes them, plus 'f' lines); ``read_ply`` / ``read_obj`` read them back.
"""
import itertools

import numpy as np

# slot s of a lattice point = the edge to cell corner SLOT_CORNER[s] (corner bits: 1 = +x, 2 = +y, 4 = +z)
SLOT_CORNER = np.array([1, 2, 4, 3, 5, 6, 7], dtype=np.int64)
_SLOT_OF_CORNER = {int(c): s for s, c in enumerate(SLOT_CORNER)}


def _corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def tet_table():
    """The case table of the kernels (hnrf_mesh.hip): (tets (6, 4) cell corners, counts (6, 16), edges (6, 16, 2, 3)).
    Tetrahedron k is (0, e_a, e_a + e_b, 7) for the k-th permutation (a, b, c) of the axes in lexicographic order; the
    mask bit i says that its vertex i is inside; an edge is coded owner corner * 8 + slot.  The winding is fixed with
    the crossings at edge midpoints: the isosurface of the linear interpolant inside a tetrahedron is planar, so it
    holds for every t."""
    tets = []
    for a, b, _ in itertools.permutations((0, 1, 2)):
        tets.append((0, 1 << a, (1 << a) | (1 << b), 7))
    counts = np.zeros((6, 16), dtype=np.int64)
    edges = np.zeros((6, 16, 2, 3), dtype=np.int64)
    for k, tv in enumerate(tets):
        for m in range(16):
            ins = [i for i in range(4) if (m >> i) & 1]
            out = [i for i in range(4) if not (m >> i) & 1]
            if len(ins) in (0, 4):
                continue

            def edge(i, j):
                u, v = min(tv[i], tv[j]), max(tv[i], tv[j])          # the corners of a Kuhn tetrahedron form a chain
                return u * 8 + _SLOT_OF_CORNER[u ^ v], (_corner_xyz(u) + _corner_xyz(v)) / 2

            if len(ins) in (1, 3):
                s = ins[0] if len(ins) == 1 else out[0]
                o = [i for i in range(4) if i != s]
                tris = [[edge(s, o[0]), edge(s, o[1]), edge(s, o[2])]]
            else:                                                    # quad ac-ad-bd-bc, split along ac-bd
                (a_, b_), (c_, d_) = ins, out
                tris = [[edge(a_, c_), edge(a_, d_), edge(b_, d_)], [edge(a_, c_), edge(b_, d_), edge(b_, c_)]]
            c_in = np.mean([_corner_xyz(tv[i]) for i in ins], axis=0)
            c_out = np.mean([_corner_xyz(tv[i]) for i in out], axis=0)
            counts[k, m] = len(tris)
            for j, t in enumerate(tris):
                n = np.cross(t[1][1] - t[0][1], t[2][1] - t[0][1])
                if np.dot(n, c_out - c_in) < 0:
                    t = [t[0], t[2], t[1]]
                edges[k, m, j] = [e[0] for e in t]
    return np.array(tets, dtype=np.int64), counts, edges


_TETS, _TRI_COUNT, _TRI_EDGES = tet_table()


def lattice_axes(bbox_min, bbox_max, N):
    """The float32 lattice coordinates along x, y, z (three arrays of N), as the kernels compute them."""
    lo = np.asarray(bbox_min, dtype=np.float32).reshape(3)
    hi = np.asarray(bbox_max, dtype=np.float32).reshape(3)
    step = (hi - lo) / np.float32(N - 1)
    i = np.arange(N, dtype=np.float32)
    return [lo[a] + i * step[a] for a in range(3)]


def _check_lattice(density, bbox_min, bbox_max):
    N = density.shape[0]
    if tuple(density.shape) != (N, N, N) or not 8 <= N <= 512:
        raise ValueError('density must be (N, N, N) with 8 <= N <= 512, got %s' % (tuple(density.shape),))
    lo = np.asarray(bbox_min, dtype=np.float32).reshape(3)
    hi = np.asarray(bbox_max, dtype=np.float32).reshape(3)
    if not np.all(hi > lo):
        raise ValueError('bbox_max must exceed bbox_min on every axis (the winding depends on it)')
    return N, lo, hi


def mesh_from_density(density, bbox_min, bbox_max, level):
    """Marching tetrahedra on the device.  density: contiguous fp32 (N, N, N) CUDA tensor.  Returns verts (V, 3)
    fp32 and faces (F, 3) int32, CUDA tensors."""
    import torch
    from . import ops
    N, lo, hi = _check_lattice(density, _host(bbox_min), _host(bbox_max))
    dev = density.device
    bmin = torch.from_numpy(lo).to(dev)
    bmax = torch.from_numpy(hi).to(dev)
    ws = ops.mesh_workspace(N, dev)
    V, F = ops.mesh_count(density, float(np.float32(level)), ws)
    return ops.mesh_emit(density, float(np.float32(level)), bmin, bmax, ws, V, F)


def _host(a):
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float32)


def mesh_from_density_host(density, bbox_min, bbox_max, level):
    """The same extraction in numpy: verts (V, 3) float32, faces (F, 3) int32, equal to the device route's."""
    d = np.ascontiguousarray(_host(density))
    N, lo, hi = _check_lattice(d, bbox_min, bbox_max)
    lv = np.float32(level)
    ins = d > lv
    flags = np.zeros((N, N, N, 7), dtype=bool)
    for s, c in enumerate(SLOT_CORNER):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        flags[:N - dz, :N - dy, :N - dx, s] = ins[:N - dz, :N - dy, :N - dx] != ins[dz:, dy:, dx:]
    flat = flags.reshape(-1)
    V = int(flat.sum())
    if V >= 2 ** 31:
        raise ValueError('%d vertices: int32 vertex ids hold at most 2^31 - 1' % V)
    vid = np.full(flat.shape, -1, dtype=np.int32)
    vid[flat] = np.arange(V, dtype=np.int32)
    vid = vid.reshape(N, N, N, 7)

    # vertices in (point, slot) order
    p, s = np.nonzero(flags.reshape(-1, 7))
    c = SLOT_CORNER[s]
    dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
    x, y, z = p % N, (p // N) % N, p // (N * N)
    dflat = d.reshape(-1)
    da = dflat[p]
    db = dflat[p + (dz * N + dy) * N + dx]
    t = (lv - da) / (db - da)
    ax = lattice_axes(lo, hi, N)
    verts = np.empty((V, 3), dtype=np.float32)
    for a, (i, di) in enumerate(((x, dx), (y, dy), (z, dz))):
        pa, pb = ax[a][i], ax[a][i + di]
        verts[:, a] = pa + t * (pb - pa)

    # triangles in (cell, tet, triangle) order, over the cells the level passes through
    M1 = N - 1
    cin = np.zeros((M1, M1, M1), dtype=np.int64)
    for k in range(8):
        cx, cy, cz = k & 1, (k >> 1) & 1, (k >> 2) & 1
        cin |= ins[cz:cz + M1, cy:cy + M1, cx:cx + M1].astype(np.int64) << k
    cz, cy, cx = np.nonzero((cin != 0) & (cin != 255))
    cin = cin[cz, cy, cx]
    n = cin.shape[0]
    tri = np.zeros((n, 6, 2, 3), dtype=np.int32)
    valid = np.zeros((n, 6, 2), dtype=bool)
    for k in range(6):
        m = np.zeros(n, dtype=np.int64)
        for i in range(4):
            m |= ((cin >> _TETS[k, i]) & 1) << i
        cnt = _TRI_COUNT[k][m]
        for j in range(2):
            valid[:, k, j] = cnt > j
            for e in range(3):
                code = _TRI_EDGES[k][m, j, e]
                u, sl = code >> 3, code & 7
                tri[:, k, j, e] = vid[cz + ((u >> 2) & 1), cy + ((u >> 1) & 1), cx + (u & 1), sl]
    faces = tri[valid]
    return verts, faces.reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------ mesh files
def _u8_colors(colors):
    """float colours in [0, 1] -> uint8 (rounded); uint8 passes through."""
    c = np.asarray(colors)
    if c.dtype == np.uint8:
        return c
    return np.clip(np.rint(c.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)


def write_ply(path, verts, faces, colors=None, normals=None):
    """Binary little-endian PLY: float x y z (+ float nx ny nz) (+ uchar red green blue), faces as 'list uchar int'.
    ``colors`` in [0, 1] (float) or uint8; ``normals`` (V, 3) float.  Without ``normals`` the file is what it always was."""
    v = np.ascontiguousarray(_host(verts)).reshape(-1, 3)
    f = np.asarray(faces.detach().cpu().numpy() if hasattr(faces, 'detach') else faces, dtype=np.int32).reshape(-1, 3)
    vfields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    if normals is not None:
        nrm = np.ascontiguousarray(_host(normals)).reshape(-1, 3)
        if nrm.shape[0] != v.shape[0]:
            raise ValueError('write_ply: %d normals for %d vertices' % (nrm.shape[0], v.shape[0]))
        vfields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
    if colors is not None:
        col = colors.detach().cpu().numpy() if hasattr(colors, 'detach') else colors
        vfields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
    vrec = np.empty(v.shape[0], dtype=vfields)
    vrec['x'], vrec['y'], vrec['z'] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        vrec['nx'], vrec['ny'], vrec['nz'] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colors is not None:
        c8 = _u8_colors(col).reshape(-1, 3)
        vrec['red'], vrec['green'], vrec['blue'] = c8[:, 0], c8[:, 1], c8[:, 2]
    frec = np.empty(f.shape[0], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    frec['n'], frec['i'] = 3, f
    header = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % v.shape[0],
              'property float x', 'property float y', 'property float z']
    if normals is not None:
        header += ['property float nx', 'property float ny', 'property float nz']
    if colors is not None:
        header += ['property uchar red', 'property uchar green', 'property uchar blue']
    header += ['element face %d' % f.shape[0], 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(header) + '\n').encode('ascii'))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path, want_normals=False):
    """Reads what ``write_ply`` writes: (verts (V,3) float32, faces (F,3) int32, colors (V,3) uint8 or None), and with
    ``want_normals`` a fourth entry, normals (V,3) float32 or None."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    lines = data[:end].decode('ascii').split('\n')
    if lines[0] != 'ply' or lines[1] != 'format binary_little_endian 1.0':
        raise ValueError('%s: not a binary little-endian PLY' % path)
    nv = nf = 0
    has_color = any(l == 'property uchar red' for l in lines)
    for l in lines:
        if l.startswith('element vertex '):
            nv = int(l.split()[2])
        elif l.startswith('element face '):
            nf = int(l.split()[2])
    has_normal = any(l == 'property float nx' for l in lines)
    vfields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')] + ([('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')] if has_normal else []) \
        + ([('r', 'u1'), ('g', 'u1'), ('b', 'u1')] if has_color else [])
    vrec = np.frombuffer(data, dtype=vfields, count=nv, offset=end)
    off = end + vrec.nbytes
    frec = np.frombuffer(data, dtype=[('n', 'u1'), ('i', '<i4', (3,))], count=nf, offset=off)
    if nf and not np.all(frec['n'] == 3):
        raise ValueError('%s: only triangles are read' % path)
    verts = np.stack([vrec['x'], vrec['y'], vrec['z']], axis=1)
    colors = np.stack([vrec['r'], vrec['g'], vrec['b']], axis=1) if has_color else None
    if want_normals:
        normals = np.stack([vrec['nx'], vrec['ny'], vrec['nz']], axis=1) if has_normal else None
        return verts, np.ascontiguousarray(frec['i']).reshape(-1, 3), colors, normals
    return verts, np.ascontiguousarray(frec['i']).reshape(-1, 3), colors


def write_obj(path, verts, faces, colors=None):
    """Wavefront OBJ: 'v x y z [r g b]' lines (colours as floats in [0, 1], the vertex-colour lines of
    render.ImageWriter.append_cnl_3d; 9 significant digits: float32 round-trips), then 1-based 'f i j k' lines."""
    v = _host(verts).reshape(-1, 3)
    f = np.asarray(faces.detach().cpu().numpy() if hasattr(faces, 'detach') else faces, dtype=np.int64).reshape(-1, 3)
    with open(path, 'w') as fh:
        if colors is None:
            fh.writelines('v %.9g %.9g %.9g\n' % tuple(p) for p in v)
        else:
            c = _host(colors).reshape(-1, 3)
            fh.writelines('v %.9g %.9g %.9g %.9g %.9g %.9g\n' % (*p, *q) for p, q in zip(v, c))
        fh.writelines('f %d %d %d\n' % tuple(t) for t in f + 1)


def read_obj(path):
    """Reads what ``write_obj`` writes: (verts (V,3) float32, faces (F,3) int32, colors (V,3) float32 or None)."""
    vs, fs = [], []
    with open(path) as fh:
        for line in fh:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == 'v':
                vs.append([float(x) for x in parts[1:]])
            elif parts[0] == 'f':
                fs.append([int(x.split('/')[0]) - 1 for x in parts[1:4]])
    va = np.array(vs, dtype=np.float32) if vs else np.zeros((0, 3), dtype=np.float32)
    faces = np.array(fs, dtype=np.int32).reshape(-1, 3)
    colors = va[:, 3:6] if va.shape[1] >= 6 else None
    return np.ascontiguousarray(va[:, :3]), faces, colors
