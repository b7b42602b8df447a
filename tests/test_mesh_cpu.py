"""Mesh extraction without a GPU: the host route of humannerf_amd.mesh on analytic fields, the mesh files, the case
table the kernels carry, and the argument checks of the new C entry points."""
import os
import re

import numpy as np
import pytest

from humannerf_amd import mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]


def field(N, f):
    ax = mesh.lattice_axes(LO, HI, N)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    return f(x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)).astype(np.float32)


def sphere(N, r):
    return field(N, lambda x, y, z: r - np.sqrt(x * x + y * y + z * z))


def edges(faces):
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])


def check_closed_manifold(verts, faces):
    """Every undirected edge in exactly two faces, every directed edge in one; returns the Euler characteristic."""
    assert faces.dtype == np.int32 and faces.min() >= 0 and faces.max() < len(verts)
    e = edges(faces)
    _, n_dir = np.unique(e, axis=0, return_counts=True)
    und, n_und = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
    assert set(n_und.tolist()) == {2}
    assert set(n_dir.tolist()) == {1}
    assert len(np.unique(faces)) == len(verts)          # no unused vertex
    return len(verts) - len(und) + len(faces)


def signed_volume(verts, faces):
    v = verts.astype(np.float64)
    return np.einsum('ij,ij->i', v[faces[:, 0]], np.cross(v[faces[:, 1]], v[faces[:, 2]])).sum() / 6.0


def test_sphere_is_closed_accurate_and_outward():
    N = 96
    step = 2.0 / (N - 1)
    R = 0.4 * (N - 1) * step
    verts, faces = mesh.mesh_from_density_host(sphere(N, R), LO, HI, 0.0)
    assert verts.dtype == np.float32 and len(faces) > 1000
    assert check_closed_manifold(verts, faces) == 2
    assert np.abs(np.linalg.norm(verts.astype(np.float64), axis=1) - R).max() <= 0.05 * step
    vol = signed_volume(verts, faces)
    assert vol > 0 and abs(vol / (4.0 / 3.0 * np.pi * R ** 3) - 1.0) < 0.01
    # winding: every face normal points away from the centre (toward lower density)
    v = verts.astype(np.float64)
    n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    c = (v[faces[:, 0]] + v[faces[:, 1]] + v[faces[:, 2]]) / 3
    assert np.all(np.einsum('ij,ij->i', n, c) > 0)


def test_torus_and_two_spheres():
    torus = field(64, lambda x, y, z: 0.04 - (np.sqrt(x * x + y * y) - 0.5) ** 2 - z * z)
    assert check_closed_manifold(*mesh.mesh_from_density_host(torus, LO, HI, 0.0)) == 0
    two = field(64, lambda x, y, z: np.maximum(0.3 - np.sqrt((x - 0.45) ** 2 + y * y + z * z),
                                               0.3 - np.sqrt((x + 0.45) ** 2 + y * y + z * z)))
    verts, faces = mesh.mesh_from_density_host(two, LO, HI, 0.0)
    assert check_closed_manifold(verts, faces) == 4
    assert np.sum(verts[:, 0] > 0) == np.sum(verts[:, 0] < 0)     # (mirror-symmetric lattice and field)


@pytest.mark.parametrize('value', [-1.0, 1.0])
def test_empty_and_full_lattices_have_no_faces(value):
    verts, faces = mesh.mesh_from_density_host(np.full((16, 16, 16), value, np.float32), LO, HI, 0.0)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


def test_level_on_lattice_values():
    d = np.rint(sphere(32, 0.6) * 4.0)          # many lattice values equal the level exactly
    assert np.sum(d == 1.0) > 100
    verts, faces = mesh.mesh_from_density_host(d, LO, HI, 1.0)
    assert np.all(np.isfinite(verts))
    assert check_closed_manifold(verts, faces) == 2


def test_surface_open_at_the_lattice_boundary():
    # a half space x < 0.1: the cut plane meets the boundary, so its edges there are in one face only
    verts, faces = mesh.mesh_from_density_host(field(16, lambda x, y, z: 0.1 - x), LO, HI, 0.0)
    _, n_und = np.unique(np.sort(edges(faces), axis=1), axis=0, return_counts=True)
    assert set(n_und.tolist()) == {1, 2}
    assert np.allclose(verts[:, 0], 0.1, atol=1e-6)


def test_single_point_star_and_vertex_order():
    """One inside lattice point: its star in the Kuhn triangulation, 14 edges and 24 tetrahedra, gives 14 vertices
    at the edge midpoints, in (owning point, slot) order, and 24 triangles."""
    N, c = 8, (3, 4, 2)                              # (z, y, x)
    d = np.zeros((N, N, N), np.float32)
    d[c] = 1.0
    verts, faces = mesh.mesh_from_density_host(d, LO, HI, 0.5)
    ax = mesh.lattice_axes(LO, HI, N)
    pos = lambda z, y, x: np.array([ax[0][x], ax[1][y], ax[2][z]], np.float32)
    want = []
    for q in np.ndindex(N, N, N):                    # (z, y, x) in point-index order
        for corner in mesh.SLOT_CORNER:
            b = (q[0] + (corner >> 2 & 1), q[1] + (corner >> 1 & 1), q[2] + (corner & 1))
            if max(b) < N and (q == c) != (b == c):
                pa, pb = pos(*q), pos(*b)
                want.append(pa + np.float32(0.5) * (pb - pa))
    assert len(want) == 14 and np.array_equal(verts, np.array(want))
    assert len(faces) == 24 and check_closed_manifold(verts, faces) == 2


def test_ply_and_obj_round_trip(tmp_path):
    verts, faces = mesh.mesh_from_density_host(sphere(20, 0.6), LO, HI, 0.0)
    colors = np.random.RandomState(0).uniform(size=verts.shape).astype(np.float32)
    mesh.write_ply(str(tmp_path / 'a.ply'), verts, faces, colors)
    v, f, c = mesh.read_ply(str(tmp_path / 'a.ply'))
    assert np.array_equal(v, verts) and np.array_equal(f, faces)
    assert np.array_equal(c, np.rint(colors.astype(np.float64) * 255).astype(np.uint8))
    mesh.write_ply(str(tmp_path / 'b.ply'), verts, faces)
    v, f, c = mesh.read_ply(str(tmp_path / 'b.ply'))
    assert np.array_equal(v, verts) and np.array_equal(f, faces) and c is None
    mesh.write_obj(str(tmp_path / 'a.obj'), verts, faces, colors)
    v, f, c = mesh.read_obj(str(tmp_path / 'a.obj'))
    assert np.array_equal(v, verts) and np.array_equal(f, faces) and np.array_equal(c, colors)
    with open(str(tmp_path / 'a.obj')) as fh:
        first = fh.readline().split()
    assert first[0] == 'v' and len(first) == 7


def test_kernel_case_table_is_the_host_table():
    """hnrf_mesh.hip carries the case table as literals; they are the ones mesh.tet_table generates."""
    with open(os.path.join(ROOT, 'humannerf_amd', 'csrc', 'hnrf_mesh.hip')) as f:
        src = f.read()

    def literal(name):
        m = re.search(r'__constant__ unsigned char ' + name + r'[^=]*=\s*(\{.*?\});', src, re.S)
        return [int(v) for v in re.findall(r'\d+', m.group(1))]
    tets, counts, tri_edges = mesh.tet_table()
    assert literal('c_slot_corner') == mesh.SLOT_CORNER.tolist()
    assert literal('c_tet') == tets.ravel().tolist()
    assert literal('c_tri_count') == counts.ravel().tolist()
    assert literal('c_tri_edges') == tri_edges.ravel().tolist()


def test_bad_lattices_are_refused():
    with pytest.raises(ValueError):
        mesh.mesh_from_density_host(np.zeros((4, 4, 4), np.float32), LO, HI, 0.0)
    with pytest.raises(ValueError):
        mesh.mesh_from_density_host(np.zeros((16, 16, 8), np.float32), LO, HI, 0.0)
    with pytest.raises(ValueError):
        mesh.mesh_from_density_host(np.zeros((16, 16, 16), np.float32), HI, LO, 0.0)


def test_mesh_abi_argument_errors_do_not_need_a_gpu():
    from humannerf_amd import _lib
    lib = _lib.load()
    err = lambda: lib.hnrf_last_error().decode()
    assert lib.hnrf_density_grid_workspace_bytes(7) == 0 and lib.hnrf_density_grid_workspace_bytes(513) == 0
    assert lib.hnrf_mesh_workspace_bytes(7) == 0 and lib.hnrf_mesh_workspace_bytes(513) == 0
    assert lib.hnrf_mesh_workspace_bytes(256) >= 256 ** 3 * 4
    ws = 1 << 12     # (a fake, aligned device address: every call below fails its checks before any launch)
    big = 1 << 40
    assert lib.hnrf_density_grid(None, 0, ws, 24, 32, ws, ws, ws, 64, ws, big, ws, None, None, None) == -1
    assert 'null pointer' in err()
    assert lib.hnrf_density_grid(ws, 0, ws, 24, 32, ws, ws, ws, 7, ws, big, ws, None, None, None) == -1
    assert 'out of range' in err()
    assert lib.hnrf_density_grid(ws, 0, ws, 24, 32, ws, ws, ws, 513, ws, big, ws, None, None, None) == -1
    assert lib.hnrf_density_grid(ws, 5, ws, 24, 32, ws, ws, ws, 64, ws, big, ws, None, None, None) == -2
    assert lib.hnrf_density_grid(ws, 0, ws, 24, 32, ws, ws, ws, 64, ws, 16, ws, None, None, None) == -4
    assert lib.hnrf_density_grid(ws, 0, ws, 24, 32, ws, ws, ws, 64, ws + 4, big, ws, None, None, None) == -1
    assert 'aligned' in err()
    assert lib.hnrf_mesh_count(None, 64, 0.0, ws, big, ws, None) == -1 and 'null pointer' in err()
    assert lib.hnrf_mesh_count(ws, 600, 0.0, ws, big, ws, None) == -1 and 'out of range' in err()
    assert lib.hnrf_mesh_count(ws, 64, float('nan'), ws, big, ws, None) == -1 and 'finite' in err()
    assert lib.hnrf_mesh_count(ws, 64, 0.0, ws, 16, ws, None) == -4
    assert lib.hnrf_mesh_emit(ws, 64, 0.0, ws, ws, ws, big, 10, 10, None, ws, None) == -1
    assert 'null output' in err()
    assert lib.hnrf_mesh_emit(ws, 4, 0.0, ws, ws, ws, big, 10, 10, ws, ws, None) == -1 and 'out of range' in err()
    assert lib.hnrf_mesh_emit(ws, 64, 0.0, ws, ws, ws, big, 1 << 31, 10, ws, ws, None) == -1
    assert lib.hnrf_forward_skin(None, 10, ws, ws, ws, 24, 32, ws, ws, ws, None) == -1 and 'null pointer' in err()
    assert lib.hnrf_forward_skin(ws, 10, ws, ws, ws, 129, 32, ws, ws, ws, None) == -1 and 'bad dims' in err()
    assert lib.hnrf_forward_skin(ws, -1, ws, ws, ws, 24, 32, ws, ws, ws, None) == -1
