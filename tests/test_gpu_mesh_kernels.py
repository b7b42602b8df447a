"""The mesh kernels of hnrf_mesh.hip -- marching tetrahedra, the density lattice's gate, forward skinning -- at the
sizes and edges tests/test_gpu_mesh.py leaves out (mesh extraction, lists which test covers which).

Problems and references: tests/test_mesh_kernel_refs.py (plain torch / numpy on the CPU, checked there without a GPU).
Marching tetrahedra is compared with the host route bit for bit.  Tolerances of the other two: 4 x the error of the
reference's own fp32 evaluation against its fp64 evaluation on the same inputs (at least 2e-7 of the quantity's scale),
computed here; where tests/test_gpu_mesh.py states a tolerance for the same quantity, the smaller of the two.  Every
comparison prints its ratio of kernel error to that floor (``pytest -s``; profiles/mesh_kernel_tests.txt has the values
of one run)."""
import numpy as np
import pytest
import torch

from tests import test_mesh_kernel_refs as mrefs
from tests import test_render_kernel_refs as refs

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _check(name, got, ref64, ref32, sel=None, cap=None):
    """max |got - ref64| <= 4 x floor (refs.tolerance), optionally capped by an older test's tolerance."""
    tol, floor = refs.tolerance(ref32, ref64, sel)
    g, r = torch.as_tensor(got).double().reshape(ref64.shape), ref64.double()
    if sel is not None:
        g, r = g[sel], r[sel]
    err = float((g - r).abs().max()) if r.numel() else 0.0
    if cap is not None:
        tol = min(tol, cap)
    print('RATIO %s err %.3e floor %.3e ratio %.2f' % (name, err, floor, err / floor if floor else 0.0))
    assert bool(torch.isfinite(g).all()), name
    assert err <= tol, (name, err, tol, floor)


# ------------------------------------------------------------------------------------------------ 1. marching tetrahedra
def _same_mesh(dev_mesh, host_mesh, nonfinite=False):
    v, f = (t.cpu().numpy() for t in dev_mesh)
    vh, fh = host_mesh
    assert f.dtype == np.int32 and f.shape == fh.shape and np.array_equal(f, fh)
    assert v.shape == vh.shape
    if nonfinite:
        assert np.array_equal(np.isnan(v), np.isnan(vh)) and np.array_equal(v, vh, equal_nan=True)
    else:
        assert np.array_equal(v.view(np.uint32), vh.view(np.uint32))


@pytest.mark.parametrize('name', mrefs.MT_CASES)
def test_device_route_equals_host_route(name):
    """mesh.mesh_from_density against mesh.mesh_from_density_host, faces equal and vertices equal as bit patterns:
    lattices whose point count is no multiple of the 256-thread block (and whose block count is no multiple of the
    1024-wide scan), random fields with every tetrahedron case, surfaces cut by the lattice boundary, single inside
    points in the corners, on a face, on an edge and under the last block, and non-finite lattice values."""
    from humannerf_amd import mesh
    c = mrefs.mt_case(name)
    with np.errstate(invalid='ignore'):
        host = mrefs.host_mesh(c)
    got = mesh.mesh_from_density(T(c['d']), c['bmin'], c['bmax'], c['level'])
    print('RATIO mt %s N %d V %d F %d' % (name, c['d'].shape[0], len(host[0]), len(host[1])))
    _same_mesh(got, host, c['nonfinite'])


@pytest.mark.parametrize('name', mrefs.DIRTY_CASES)
def test_extraction_does_not_read_what_it_has_not_written(name):
    """hnrf_mesh_count / hnrf_mesh_emit on a workspace filled with 0xFF bytes and on one filled with zeros: the same
    counts and the same bits (and the host route's)."""
    from humannerf_amd import ops
    c = mrefs.mt_case(name)
    d, N = T(c['d']), c['d'].shape[0]
    bmin, bmax = T(np.array(c['bmin'], np.float32)), T(np.array(c['bmax'], np.float32))
    runs = []
    for fill in (0xFF, 0x00):
        ws = ops.mesh_workspace(N, dev())
        ws.view(torch.uint8).fill_(fill)
        V, F = ops.mesh_count(d, c['level'], ws)
        v, f = ops.mesh_emit(d, c['level'], bmin, bmax, ws, V, F)
        runs.append((V, F, v.cpu().numpy(), f.cpu().numpy()))
    assert runs[0][:2] == runs[1][:2]
    assert np.array_equal(runs[0][2].view(np.uint32), runs[1][2].view(np.uint32)) and np.array_equal(runs[0][3], runs[1][3])
    _same_mesh((torch.from_numpy(runs[0][2]), torch.from_numpy(runs[0][3])), mrefs.host_mesh(c))


# ------------------------------------------------------------------------------------------------ 2. the density lattice
@pytest.fixture(scope='module')
def net():
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state, with_density
    state = with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0)
    n = Network()
    n.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return n.to(dev()).eval()


@pytest.fixture(scope='module')
def frame():
    from humannerf_amd import scene
    return scene.synthetic_frame(H=64, W=64, pose_seed=3, pose_scale=0.3)


@pytest.fixture
def mode_is():
    from humannerf_amd.config import cfg
    old = cfg.amd.mlp_mode

    def set_mode(m):
        cfg.amd.mlp_mode = m
    yield set_mode
    cfg.amd.mlp_mode = old


@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
def test_density_grid_across_a_chunk_boundary(net, frame, mode, mode_is):
    """N = 129: two chunks of hnrf_density_grid, the second with 49 537 points.  sigma equals the canonical kernel on
    the lattice points bit for bit, density = relu(sigma) * fg bit for bit, and fg matches fp64 on every 97th point,
    on the 1 024 points on each side of the chunk boundary and on the last 1 024."""
    from humannerf_amd import ops
    mode_is(mode)
    N = 129
    bmin, bmax = frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz']
    density, sigma, fg = net.canonical_density_grid(bmin, bmax, frame['motion_weights_priors'], resolution=N,
                                                    cnl_bbox_scale_xyz=frame['cnl_bbox_scale_xyz'], return_parts=True)
    assert density.shape == (N, N, N)
    pts = mrefs.lattice_points(bmin, bmax, N)
    raw = ops.canonical(T(pts), net._canonical_packed(), mode)
    assert torch.equal(sigma.reshape(-1), raw[:, 3])
    assert torch.equal(density, torch.relu(sigma) * fg)
    with torch.no_grad():
        vol = net._weight_volume(T(frame['motion_weights_priors'])).cpu().numpy()
    idx = mrefs.fg_subset(N)
    B = vol.shape[0] - 1
    r64 = mrefs.ref_fg(vol, B, bmin, frame['cnl_bbox_scale_xyz'], pts[idx])
    r32 = mrefs.ref_fg(vol, B, bmin, frame['cnl_bbox_scale_xyz'], pts[idx], torch.float32)
    got = fg.reshape(-1)[T(idx)].cpu()
    assert float(r64.max()) > 0.5 and float(r64.min()) < 1e-3          # the gate does cut the lattice
    for tag, sel in (('all', slice(None)), ('chunk-edge', (idx >= (1 << 21) - 1024) & (idx < (1 << 21) + 1024)),
                     ('tail', idx >= N ** 3 - 1024)):
        sel = torch.ones(len(idx), dtype=torch.bool) if tag == 'all' else torch.from_numpy(sel)
        _check('fg N129 %s %s' % (mode, tag), got, r64, r32, sel=sel, cap=1e-6)


def test_density_grid_outside_the_weight_volume(net, mode_is):
    """ops.density_grid called directly at N = 8 with a volume (B = 3, G = 5) that ends half way along the lattice
    box: where every corner is zero-padded fg and density are exactly 0; elsewhere fg against fp64."""
    from humannerf_amd import ops
    mode_is('f32')
    pr, all_out = mrefs.fg_outside_problem()
    with torch.no_grad():
        density, sigma, fg = ops.density_grid(net._canonical_packed(), T(pr['vol']), T(pr['bmin']), T(pr['bmax']),
                                              T(pr['bscale']), pr['N'], 'f32', want_parts=True)
    torch.cuda.synchronize()
    fg, density, sigma = fg.reshape(-1).cpu(), density.reshape(-1).cpu(), sigma.reshape(-1).cpu()
    out = torch.from_numpy(all_out)
    assert float(out.double().mean()) >= 0.25
    assert bool((fg[out] == 0).all()) and bool((density[out] == 0).all())
    assert bool((sigma[out] > 0).any())                               # (it is the gate that zeroes them)
    assert torch.equal(density, torch.relu(sigma) * fg)
    r64 = mrefs.ref_fg(pr['vol'], pr['B'], pr['bmin'], pr['bscale'], pr['pts'])
    r32 = mrefs.ref_fg(pr['vol'], pr['B'], pr['bmin'], pr['bscale'], pr['pts'], torch.float32)
    _check('fg outside N8 B3 G5', fg, r64, r32, cap=1e-6)


# ------------------------------------------------------------------------------------------------ 3. forward skinning
def _skin(pr):
    from humannerf_amd import ops
    out = ops.forward_skin(*(T(pr[k]) for k in ('verts', 'Rs', 'Ts', 'vol', 'bmin', 'bscale')))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('case', mrefs.SKIN_CASES, ids=lambda c: 'B%d_G%d_V%d' % c)
def test_forward_skin_against_fp64(case):
    """hnrf_forward_skin at every shape of mrefs.SKIN_CASES: the numerator out * max(sum w, 1e-4) on EVERY vertex (it
    has no conditioning problem), out itself where sum w >= 1e-2 (at least 70 % of a problem: asserted from the
    reference), and exactly 0 where every corner is zero-padded."""
    pr = mrefs.skin_problem(*case)
    r64, r32 = mrefs.ref_skin(pr), mrefs.ref_skin(pr, torch.float32)
    out = _skin(pr)
    tag = 'skin B%d G%d V%d ' % case
    zero = torch.from_numpy(pr['all_out'])
    assert bool((out[zero] == 0).all())
    num = out.double() * r64['wsum'].clamp(min=1e-4)[:, None]
    _check(tag + 'num', num, r64['num'], r32['num'])
    ok = r64['wsum'] >= 1e-2
    assert float(ok.double().mean()) >= mrefs.SKIN_MIN_SHARE
    _check(tag + 'out', out, r64['out'], r32['out'], sel=ok[:, None].expand(-1, 3), cap=1e-5)


@pytest.mark.parametrize('case', mrefs.SKIN_CLAMP_CASES, ids=lambda c: 'B%d_G%d_V%d' % c)
def test_forward_skin_inside_the_clamp_of_the_weight_sum(case):
    """Planted: the whole volume scaled by 2e-6, so that 0 < sum w < 1e-4 wherever a vertex meets the lattice and out =
    numerator / 1e-4: the clamp decides the value, and out is compared on every vertex."""
    pr = mrefs.skin_problem(*case, vol_scale=2e-6)
    r64, r32 = mrefs.ref_skin(pr), mrefs.ref_skin(pr, torch.float32)
    assert float(r64['wsum'].max()) < 1e-4 and float((r64['wsum'] > 0).double().mean()) > 0.5
    out = _skin(pr)
    assert bool((out[torch.from_numpy(pr['all_out'])] == 0).all())
    _check('skin-clamp B%d G%d V%d out' % case, out, r64['out'], r32['out'])


@pytest.mark.parametrize('B', [24, 7])
def test_forward_skin_exact_lattice_cases(B):
    """mrefs.skin_exact_problem: identity bones, every vertex a lattice node or the midpoint of 2 / 4 / 8 nodes, from
    one and a half cells outside to one and a half cells outside.  In exact fp32 arithmetic (asserted on the formula's
    fp32 statement in tests/test_mesh_kernel_refs.py) the vertex comes back BIT FOR BIT where sum w >= 1e-4, as
    x * sum w / 1e-4 below that, and as exactly 0 from a whole cell outside on."""
    f = np.float32
    pr, lat = mrefs.skin_exact_problem(B)
    want, wsum = mrefs.skin_statement_fp32(pr, lat)
    out = _skin(pr).numpy()
    x = pr['verts']
    hi = wsum >= f(0.0001)
    low = ~hi & (wsum > 0)
    out_cell = ((lat <= -1) | (lat >= mrefs.SKIN_EXACT_G)).any(1)
    print('RATIO skin-exact B%d vertices %d: sum w >= 1e-4 on %d, inside (0, 1e-4) on %d, a cell or more outside %d' %
          (B, len(x), hi.sum(), low.sum(), out_cell.sum()))
    bad = np.argwhere(out.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (len(bad), lat[bad[0][0]].tolist(), out[bad[0][0]].tolist(), want[bad[0][0]].tolist())
    assert np.array_equal(out[hi], x[hi])
    assert np.array_equal(out[low], ((x[low] * wsum[low, None]).astype(f) / f(0.0001)).astype(f))
    assert hi.any() and low.any() and out_cell.any() and (out[out_cell] == 0).all()
