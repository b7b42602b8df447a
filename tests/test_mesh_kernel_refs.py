"""Problem builders and fp64 references of the mesh kernels (tests/test_gpu_mesh_kernels.py): marching tetrahedra at
ragged sizes, on surfaces that reach the lattice boundary and on non-finite lattices; the gate of hnrf_density_grid
across a chunk boundary and outside the weight volume; hnrf_forward_skin; and the checks of those builders that need no
GPU.  Every reference is plain torch / numpy on the CPU; ``dtype`` selects fp64 (the reference) or fp32 (the same
expressions in the kernels' precision: its distance from fp64 is the noise floor the GPU tests scale their tolerances
by, tests/test_render_kernel_refs.py::tolerance)."""
import numpy as np
import pytest
import torch

from humannerf_amd import mesh
from humannerf_amd.network import rodrigues
from oracle import oracle
from tests import test_render_kernel_refs as refs

CUBE = ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0])
ANISO = ([-0.7, -1.3, 0.1], [0.9, 0.2, 0.35])
BLOCK = 256                                  # threads of mesh_count_kernel / mesh_emit_kernel / forward_skin_kernel


# ------------------------------------------------------------------------------------------------ marching tetrahedra
def field(N, f, box=CUBE):
    ax = mesh.lattice_axes(box[0], box[1], N)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    return f(x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)).astype(np.float32)


def sphere(N, r):
    return field(N, lambda x, y, z: r - np.sqrt(x * x + y * y + z * z))


RAGGED_N = [8, 9, 17, 33, 65, 129]           # blocks: 2 (exact), 3 (last 217), 20, 141, 1 073, 8 386 (last: 129 points)
RANDOM_N = [8, 9, 12]
HALF_SPACES = [(axis, sign) for axis in range(3) for sign in (1, -1)]
OPEN_SPHERE_N = [11, 17]
STAR_N = 9
# name -> (z, y, x) of the one inside point
STARS = {'inner': (STAR_N - 2,) * 3, 'last': (STAR_N - 1,) * 3, 'first': (0, 0, 0),
         'face': (STAR_N // 2, STAR_N // 2, STAR_N - 1), 'edge': (STAR_N - 1, STAR_N - 1, STAR_N // 2)}
# (z, y, x) -> planted value on the N = 9 sphere of radius 0.8 (nodes at multiples of 0.25; centre (4, 4, 4))
NONFINITE_PLANTS = {(4, 5, 6): np.nan,       # an inside point (0.24 under the surface) turned outside
                    (1, 1, 1): np.inf,       # an outside point turned inside: all its neighbours are finite
                    (7, 7, 6): np.inf, (7, 7, 7): np.inf,      # two adjacent: no vertex on the edge between them
                    (4, 4, 3): -np.inf}      # an inside point turned outside


def mt_case(name):
    """name -> dict(d (N, N, N) fp32, bmin, bmax, level, nonfinite).  Names: ragged-N, random-N, half-<axis><+|->,
    open-sphere-N, star-<name>, nonfinite."""
    kind, _, arg = name.partition('-')
    box, level, nonfinite = CUBE, 0.0, False
    if kind == 'ragged':
        d = sphere(int(arg), 0.8)
    elif kind == 'random':
        N = int(arg)
        d, box, level = np.random.RandomState(100 + N).randn(N, N, N).astype(np.float32), ANISO, 0.1
    elif kind == 'half':
        axis, sign = 'xyz'.index(arg[0]), 1.0 if arg[1] == '+' else -1.0
        d = field(11, lambda x, y, z: sign * (0.13 - (x, y, z)[axis]))
    elif kind == 'open':
        d = sphere(int(arg.split('-')[1]), 1.2)
    elif kind == 'star':
        d, level = np.zeros((STAR_N,) * 3, np.float32), 0.5
        d[STARS[arg]] = 1.0
    elif kind == 'nonfinite':
        d, nonfinite = sphere(9, 0.8), True
        for q, v in NONFINITE_PLANTS.items():
            d[q] = v
    else:
        raise KeyError(name)
    return dict(d=np.ascontiguousarray(d), bmin=box[0], bmax=box[1], level=level, nonfinite=nonfinite)


RAGGED_CASES = ['ragged-%d' % N for N in RAGGED_N]
RANDOM_CASES = ['random-%d' % N for N in RANDOM_N]
OPEN_CASES = ['half-%s%s' % ('xyz'[a], '+' if s > 0 else '-') for a, s in HALF_SPACES] + \
             ['open-sphere-%d' % N for N in OPEN_SPHERE_N]
STAR_CASES = ['star-' + k for k in STARS]
MT_CASES = RAGGED_CASES + RANDOM_CASES + OPEN_CASES + STAR_CASES + ['nonfinite']
DIRTY_CASES = ['ragged-9', 'open-sphere-11']


def host_mesh(c):
    return mesh.mesh_from_density_host(c['d'], c['bmin'], c['bmax'], c['level'])


def tet_masks(d, level):
    """The set of (tetrahedron, inside mask) pairs over all cells of a lattice."""
    tets, _, _ = mesh.tet_table()
    ins = d > np.float32(level)
    M1 = d.shape[0] - 1
    corner = [ins[(k >> 2) & 1:((k >> 2) & 1) + M1, (k >> 1) & 1:((k >> 1) & 1) + M1, (k & 1):(k & 1) + M1] for k in range(8)]
    seen = set()
    for k in range(6):
        m = sum(corner[tets[k, i]].astype(np.int64) << i for i in range(4))
        seen |= {(k, int(v)) for v in np.unique(m)}
    return seen


def star_counts(q, N):
    """(vertices, triangles) of one inside lattice point q = (z, y, x), counted from the Kuhn triangulation alone: one
    vertex per lattice edge of its star that lies in the lattice (the 14 neighbours +-(1,0,0) ... +-(1,1,1) with equal
    signs), one triangle per tetrahedron that has q as a corner -- as corner c of the cell at q - c: all six
    tetrahedra for c = 0 and 7, two each for the other corners."""
    tets, _, _ = mesh.tet_table()
    z, y, x = q
    nv = 0
    for c in range(1, 8):
        for s in (1, -1):
            b = (x + s * (c & 1), y + s * ((c >> 1) & 1), z + s * ((c >> 2) & 1))
            nv += all(0 <= v < N for v in b)
    nt = 0
    for c in range(8):
        o = (x - (c & 1), y - ((c >> 1) & 1), z - ((c >> 2) & 1))
        if all(0 <= v < N - 1 for v in o):
            nt += sum(c in t.tolist() for t in tets)
    return nv, nt


# ------------------------------------------------------------------------------------------------ the gate fg
def lattice_points(bmin, bmax, N):
    ax = mesh.lattice_axes(bmin, bmax, N)
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    return np.stack([x, y, z], -1).reshape(-1, 3)


def ref_fg(vol, B, bmin, bscale, pts, dtype=torch.float64):
    """fg of hnrf_density_grid at ``pts`` (P, 3): the sum over the B bone channels of oracle.trilinear_zeros."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    g = (t(pts) - t(bmin)[None]) * t(bscale)[None] - 1.0
    v = t(vol)
    out = torch.zeros(len(pts), dtype=dtype)
    for b in range(B):
        out = out + oracle.trilinear_zeros(v[b], g)
    return out


def fg_subset(N, chunk=1 << 21):
    """Indices of the lattice points whose fg is compared with fp64 at N = 129: every 97th, the 1 024 on each side of
    the chunk boundary of hnrf_density_grid, the last 1 024."""
    M = N ** 3
    assert chunk + 1024 <= M - 1024
    return np.unique(np.concatenate([np.arange(0, M, 97), np.arange(chunk - 1024, chunk + 1024), np.arange(M - 1024, M)]))


def fg_outside_problem():
    """A direct hnrf_density_grid call at N = 8 with B = 3, G = 5: the entry places the weight volume at bbox_min, and
    bbox_scale makes it end half way along every axis of the lattice box, so that the lattice points past the middle
    read zero padding.  Returns the problem and ``all_out``: the points whose 8 corners are all out of range (decided
    in fp64, at least a quarter of a cell from the edge of that set)."""
    rs = np.random.RandomState(4)
    N, B, G = 8, 3, 5
    bmin, bmax = np.array(ANISO[0], np.float32), np.array(ANISO[1], np.float32)
    bscale = (4.0 / (bmax.astype(np.float64) - bmin)).astype(np.float32)
    vol = rs.uniform(0.05, 1.0, (B + 1, G, G, G)).astype(np.float32)
    pts = lattice_points(bmin, bmax, N)
    lat = (pts.astype(np.float64) - bmin) * bscale.astype(np.float64) * 0.5 * (G - 1)      # node i at lat = i
    assert (np.abs(lat - G) > 0.25).all() and (np.abs(lat - (G - 1)) > 0.25).all() and lat.min() > -0.25
    all_out = (lat > G).any(1)
    return dict(N=N, B=B, G=G, bmin=bmin, bmax=bmax, bscale=bscale, vol=vol, pts=pts), all_out


# ------------------------------------------------------------------------------------------------ forward skinning
SKIN_BMIN = np.array([-1.0, -1.2, -0.4], np.float32)
SKIN_EXTENT = np.array([2.0, 2.4, 0.8])
# (B, G, V): every B, G and V of the issue once or more; B = 128 fills the kernel's table, 25 is one past the common 24
SKIN_CASES = [(1, 2, 1), (7, 3, 255), (24, 32, 256), (25, 33, 257), (128, 32, 1000), (24, 2, 1000), (128, 3, 257),
              (7, 33, 1000)]
SKIN_CLAMP_CASES = [SKIN_CASES[1], SKIN_CASES[3], SKIN_CASES[4]]
SKIN_MIN_SHARE = 0.70


def skin_problem(B, G, V, seed=3, vol_scale=1.0):
    """Inputs of hnrf_forward_skin (numpy fp32) on an anisotropic box: rotations by up to pi, translations within +-2,
    a softmax volume with the background channel last.  Vertices: inside the volume; then, where V allows, within one
    cell outside a face (some corners zero-padded), 1.25 to 3 cells outside on one, two and three axes (every corner
    zero-padded: ``all_out``), and 1e6 away (the int conversion clamped).  ``vol_scale``: factor on the whole volume
    (2e-6: every weight sum lies under the 1e-4 clamp)."""
    gen = torch.Generator().manual_seed(seed + 1000 * B + 10 * G + V)
    rs = np.random.RandomState(seed + 7 * B + 3 * G + V)
    axis = rs.randn(B, 3)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = rs.uniform(0.0, np.pi, (B, 1))
    angle[0] = np.pi
    Rs = rodrigues(torch.from_numpy(axis * angle)).numpy().astype(np.float32)
    Ts = rs.uniform(-2.0, 2.0, (B, 3)).astype(np.float32)
    vol = (torch.softmax(torch.randn(B + 1, G, G, G, generator=gen, dtype=torch.float64) * 3.0, dim=0).numpy()
           * vol_scale).astype(np.float32)
    cell = SKIN_EXTENT / (G - 1)
    u = rs.uniform(0.0, 1.0, (V, 3))                             # position in units of the box
    kind = np.zeros(V, np.int64)                                 # 0 inside, 1 face, 2..4 outside on 1..3 axes, 5 far
    if V >= 255:
        n_face, n_out, n_far = int(0.06 * V), int(0.025 * V), max(1, int(0.015 * V))
        at = V - (n_face + 3 * n_out + n_far)
        side = lambda n: rs.choice([-1.0, 1.0], n)

        def push(rows, axes, lo, hi):                            # move rows ``lo``..``hi`` cells past a face on ``axes``
            for a in axes:
                s, k = side(len(rows)), rs.uniform(lo, hi, len(rows))
                u[rows, a] = np.where(s > 0, 1.0 + k * cell[a] / SKIN_EXTENT[a], -k * cell[a] / SKIN_EXTENT[a])
        rows = np.arange(at, at + n_face)
        push(rows, [0], 0.05, 0.95), push(rows[::3], [1], 0.05, 0.95), push(rows[::5], [2], 0.05, 0.95)
        kind[rows], at = 1, at + n_face
        for n_axes in (1, 2, 3):
            rows = np.arange(at, at + n_out)
            push(rows, [(n_axes + j) % 3 for j in range(n_axes)], 1.25, 3.0)
            kind[rows], at = 1 + n_axes, at + n_out
        kind[at:] = 5
    verts = (SKIN_BMIN.astype(np.float64) + u * SKIN_EXTENT).astype(np.float32)
    far = np.nonzero(kind == 5)[0]
    verts[far] = (rs.choice([-1e6, 1e6], (len(far), 3))).astype(np.float32)
    if len(far) > 1:
        verts[far[1], 1:] = [0.1, -0.1]                          # far on one axis only
    return dict(verts=verts, Rs=Rs, Ts=Ts, vol=vol, bmin=SKIN_BMIN, bscale=(2.0 / SKIN_EXTENT).astype(np.float32),
                B=B, G=G, V=V, kind=kind, all_out=kind >= 2)


def ref_skin(pr, dtype=torch.float64):
    """The expression of tests/test_gpu_mesh.py::test_pose_vertices_on_a_synthetic_pose in ``dtype``: dict(wsum (V,),
    out (V, 3), num (V, 3) = out * max(wsum, 1e-4))."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    x, Rs, Ts, vol = t(pr['verts']), t(pr['Rs']), t(pr['Ts']), t(pr['vol'])
    g = (x - t(pr['bmin'])) * t(pr['bscale']) - 1.0
    w = torch.stack([oracle.trilinear_zeros(vol[b], g) for b in range(pr['B'])], -1)
    xb = torch.einsum('bij,vbj->vbi', torch.linalg.inv(Rs), x[:, None, :] - Ts[None])
    wsum = w.sum(1)
    out = (w[..., None] * xb).sum(1) / wsum.clamp(min=1e-4)[:, None]
    return dict(wsum=wsum, out=out, num=out * wsum.clamp(min=1e-4)[:, None])


SKIN_EXACT_G = 33
# coordinates in half cells (h = 2 x lattice coordinate; the vertex coordinate is h / 32 - 1): one and a half, one and
# half a cell outside, the first nodes and midpoints (the sparse slab of the volume), the middle, and the far faces
SKIN_EXACT_H = np.array([-3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 30, 31, 32, 33, 57, 58, 61, 62, 63, 64, 65, 66, 67])


def skin_exact_problem(B):
    """Identity rotations, zero translations, box [-1, 1]^3 with scale 1, G = 33 (node i at -1 + i / 16).  The volume
    holds multiples of 2^-13 whose sum over the channels of a voxel is below 1; the slab z < 4 is empty except for
    single entries of 2^-13 (one bone) on the nodes (z, y, x) = (1, 3j, 3k), so that weight sums of 2^-13 (on such a
    node, >= 1e-4), 2^-14, 2^-15 and 2^-16 (midpoints of 2, 4, 8 nodes, < 1e-4) occur.  Vertices: the product of
    SKIN_EXACT_H on the three axes.  In fp32 every product w_b * x and every partial sum is exact.  Returns the problem
    and the lattice coordinates (V, 3)."""
    G = SKIN_EXACT_G
    rs = np.random.RandomState(17 + B)
    vol = rs.randint(1, 8192 // (B + 1), (B + 1, G, G, G)).astype(np.float64) / 8192.0
    vol[:, :4] = 0
    vol[rs.randint(0, B, (11, 11)), 1, 3 * np.arange(11)[:, None], 3 * np.arange(11)[None, :]] = 1.0 / 8192.0
    h = SKIN_EXACT_H
    hz, hy, hx = np.meshgrid(h, h, h, indexing='ij')
    lat = np.stack([hx, hy, hz], -1).reshape(-1, 3) / 2.0
    verts = (lat / 16.0 - 1.0).astype(np.float32)
    assert np.array_equal(verts.astype(np.float64), lat / 16.0 - 1.0)
    pr = dict(verts=verts, Rs=np.tile(np.eye(3, dtype=np.float32), (B, 1, 1)), Ts=np.zeros((B, 3), np.float32),
              vol=vol.astype(np.float32), bmin=np.full(3, -1.0, np.float32), bscale=np.ones(3, np.float32), B=B, G=G,
              V=len(verts))
    assert np.array_equal(pr['vol'].astype(np.float64), vol)
    return pr, lat


def skin_statement_fp32(pr, lat):
    """hnrf_forward_skin on a problem of skin_exact_problem as the kernel states it, in numpy fp32 with one rounding
    per operation: w_b exact (asserted), q_b = x (identity bone), the sums over the bones in bone order, den =
    max(sum w, 0.0001f), out = sum / den.  Returns (out (V, 3) fp32, wsum (V,) fp32)."""
    f = np.float32
    w64 = refs.exact_lattice_weights(pr['vol'][:pr['B']], lat)
    w = w64.astype(f)
    assert np.array_equal(w.astype(np.float64), w64)
    x = pr['verts']
    wsum, acc = np.zeros(len(x), f), np.zeros((len(x), 3), f)
    for b in range(pr['B']):
        wsum = (wsum + w[:, b]).astype(f)
        acc = (acc + (w[:, b, None] * x).astype(f)).astype(f)
    den = np.maximum(wsum, f(0.0001))
    return (acc / den[:, None]).astype(f), wsum


# ------------------------------------------------------------------------------------------------ checks (no GPU)
def _edges(faces):
    return np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)


def test_ragged_sizes_are_ragged():
    """The block counts the cases are chosen for: 2 exact blocks, a last block of 217, 1 073 blocks (a second pass of
    the 1024-wide block scan with 49), 8 386 blocks (a ninth pass with 194) whose last holds 129 points."""
    blocks = {N: -(-N ** 3 // BLOCK) for N in RAGGED_N}
    assert blocks[8] == 2 and 8 ** 3 % BLOCK == 0
    assert blocks[9] == 3 and 9 ** 3 % BLOCK == 217
    assert all(N % BLOCK and BLOCK % N for N in (17, 33))                       # rows straddle blocks
    assert blocks[65] == 1073 and blocks[65] - 1024 == 49
    assert blocks[129] == 8386 and blocks[129] - 8 * 1024 == 194 and 129 ** 3 % BLOCK == 129
    for N in RAGGED_N[:-1]:
        v, f = host_mesh(mt_case('ragged-%d' % N))
        assert len(f) > 100 and len(np.unique(_edges(f), axis=0)) * 2 == len(f) * 3         # closed


@pytest.mark.parametrize('name', OPEN_CASES)
def test_open_cases_are_open_only_at_the_boundary(name):
    """Every undirected edge is in one or two faces, those in one face lie on the boundary of the box, no vertex is
    unused; the half-space vertices sit on their plane."""
    c = mt_case(name)
    verts, faces = host_mesh(c)
    und, n = np.unique(_edges(faces), axis=0, return_counts=True)
    assert set(n.tolist()) == {1, 2}
    assert len(np.unique(faces)) == len(verts) and faces.min() == 0 and faces.max() == len(verts) - 1
    ax = mesh.lattice_axes(c['bmin'], c['bmax'], c['d'].shape[0])
    on_face = np.stack([(verts[:, a] == ax[a][0]) | (verts[:, a] == ax[a][-1]) for a in range(3)], 1)   # (V, 3)
    a, b = und[n == 1].T
    assert (on_face[a] & on_face[b]).any(1).all()                # both ends on one face of the box
    if name.startswith('half'):
        assert np.abs(verts[:, 'xyz'.index(name[5])] - 0.13).max() <= 1e-6
    else:
        ins = c['d'] > 0
        assert not ins[0, 0, 0] and not ins[-1, -1, -1] and ins[0, 5, 5] and ins[5, 5, -1]     # corners out, faces cut


@pytest.mark.parametrize('name', RANDOM_CASES)
def test_random_cases_hold_every_tetrahedron_case(name):
    c = mt_case(name)
    seen = tet_masks(c['d'], c['level'])
    assert seen >= {(k, m) for k in range(6) for m in range(1, 15)} and len(seen - {(k, m) for k in range(6) for m in (0, 15)}) == 84
    verts, faces = host_mesh(c)
    N = c['d'].shape[0]
    assert len(verts) > 2.5 * N ** 3 and np.isfinite(verts).all()                # (of at most 7 per point)


def test_star_cases_have_the_counts_of_the_triangulation():
    want = {'inner': (14, 24), 'last': (7, 6), 'first': (7, 6), 'face': (10, 12), 'edge': (8, 8)}
    for k, q in STARS.items():
        verts, faces = host_mesh(mt_case('star-' + k))
        assert (len(verts), len(faces)) == star_counts(q, STAR_N), k
        assert (len(verts), len(faces)) == want[k], k
    # the star of (N-2)^3 ends with the last point of the lattice, in the last, ragged block
    last = STAR_N ** 3 - 1
    assert last // BLOCK == 2 and (last + 1) % BLOCK == 217


def test_nonfinite_case_on_the_host_route():
    """NaN and -inf count as outside, +inf as inside; vertices next to them are NaN (inf / inf) or sit on the finite
    end (t = 0); the pair of +inf has no vertex between them."""
    c = mt_case('nonfinite')
    clean = sphere(9, 0.8)
    assert clean[4, 5, 6] > 0 and clean[4, 4, 3] > 0 and clean[1, 1, 1] < 0 and clean[7, 7, 6] < 0 and clean[7, 7, 7] < 0
    with np.errstate(invalid='ignore'):
        ins = c['d'] > 0
        assert ins[7, 7, 6] and ins[7, 7, 7] and ins[1, 1, 1] and not ins[4, 5, 6] and not ins[4, 4, 3]
        verts, faces = host_mesh(c)
        v0, f0 = mesh.mesh_from_density_host(clean, *CUBE, 0.0)
    assert len(verts) > len(v0) and len(faces) > len(f0)
    bad = np.isnan(verts).any(1)
    assert 0 < bad.sum() < len(verts) and not np.isinf(verts).any()
    assert len(np.unique(faces)) == len(verts)


def test_fg_outside_problem_keeps_its_share():
    pr, all_out = fg_outside_problem()
    assert all_out.mean() >= 0.25 and (~all_out).mean() >= 0.1
    fg = ref_fg(pr['vol'], pr['B'], pr['bmin'], pr['bscale'], pr['pts'])
    assert bool((fg[all_out] == 0).all()) and bool((fg[~all_out] > 0).all())
    partial = ((pr['pts'].astype(np.float64) - pr['bmin']) * pr['bscale'] * 2 > 4).any(1) & ~all_out
    assert partial.any()                                          # some points have corners on both sides


def test_fg_subset_straddles_the_chunk_boundary():
    idx = fg_subset(129)
    chunk = 1 << 21
    assert 129 ** 3 - chunk == 49537 and idx.max() == 129 ** 3 - 1
    assert ((idx >= chunk - 1024) & (idx < chunk)).sum() >= 1024 and ((idx >= chunk) & (idx < chunk + 1024)).sum() >= 1024


@pytest.mark.parametrize('case', SKIN_CASES, ids=lambda c: 'B%d_G%d_V%d' % c)
def test_skin_problems_keep_their_caps(case):
    """What the GPU test may leave out of the comparison of ``out``, from the reference alone: the vertices with a
    weight sum >= 1e-2 are at least 70 % of a problem; the vertices placed past one cell have a weight sum of exactly
    0; the planted low-weight volume puts the weight sum inside (0, 1e-4) on more than half the vertices."""
    pr = skin_problem(*case)
    r = ref_skin(pr)
    assert float((r['wsum'] >= 1e-2).double().mean()) >= SKIN_MIN_SHARE
    assert bool((r['wsum'][pr['all_out']] == 0).all()) and bool((r['out'][pr['all_out']] == 0).all())
    assert bool((r['wsum'][~pr['all_out']] > 0).all())
    if case[2] >= 255:
        assert set(pr['kind'].tolist()) == {0, 1, 2, 3, 4, 5}
        face = r['wsum'][pr['kind'] == 1]
        assert float(face.min()) < 0.5 * float(r['wsum'][pr['kind'] == 0].min()) or float(face.min()) < 1e-2
    det = np.linalg.det(pr['Rs'].astype(np.float64))
    assert np.abs(det - 1).max() < 1e-4 and np.abs(pr['Ts']).max() <= 2    # (rodrigues: theta = sqrt(1e-5 + |r|^2))
    assert np.arccos(np.clip((np.trace(pr['Rs'], axis1=1, axis2=2)[0] - 1) / 2, -1, 1)) > 3.1       # bone 0: by pi
    if case in SKIN_CLAMP_CASES:
        low = ref_skin(skin_problem(*case, vol_scale=2e-6))
        inside = (low['wsum'] > 0) & (low['wsum'] < 1e-4)
        assert float(low['wsum'].max()) < 1e-4 and float(inside.double().mean()) > 0.5


@pytest.mark.parametrize('B', [24, 7])
def test_skin_exact_problem_is_exact_in_fp32(B):
    """The three statements the GPU test relies on, on the fp32 statement of the kernel's formula: out equals the input
    bit for bit wherever sum w >= 1e-4, equals input * sum w / 1e-4 below that, and is exactly 0 from a whole cell
    outside on; and every one of the three occurs, on nodes and on midpoints."""
    f = np.float32
    pr, lat = skin_exact_problem(B)
    out, wsum = skin_statement_fp32(pr, lat)
    x = pr['verts']
    w64 = refs.exact_lattice_weights(pr['vol'][:B], lat).sum(-1)
    assert np.array_equal(wsum.astype(np.float64), w64)           # the fp32 sum over the bones is exact
    r = ref_skin(pr)
    assert float((r['wsum'] - torch.from_numpy(w64)).abs().max()) <= 1e-15
    hi = wsum >= f(0.0001)
    out_cell = ((lat <= -1) | (lat >= SKIN_EXACT_G)).any(1)
    assert np.array_equal(out[hi], x[hi])
    low = ~hi & (wsum > 0)
    assert np.array_equal(out[low], ((x[low] * wsum[low, None]).astype(f) / f(0.0001)).astype(f))
    assert (x[low].astype(np.float64) * w64[low, None] == (x[low] * wsum[low, None]).astype(np.float64)).all()
    assert (wsum[out_cell] == 0).all() and (out[out_cell] == 0).all() and (wsum[~out_cell] > 0).mean() > 0.5
    assert hi.sum() > 1000 and low.sum() > 100 and out_cell.sum() > 1000
    assert {2.0 ** -14, 2.0 ** -15, 2.0 ** -16} <= set(np.unique(w64[low]).tolist()) and (w64[hi] == 2.0 ** -13).any()
    frac = lat - np.floor(lat)
    for n_half in range(4):                                      # nodes, midpoints of 2, 4, 8 nodes: inside the clamp or not
        sel = (frac != 0).sum(1) == n_half
        assert (sel & hi).any() and (sel & out_cell).any(), n_half
    half_out = ((lat == -0.5) | (lat == SKIN_EXACT_G - 0.5)).any(1) & ~out_cell
    assert (half_out & hi).any()
    # against fp64 the statement is the reference's, to rounding
    assert float((torch.from_numpy(out).double() - r['out']).abs().max()) <= 1e-6
