"""Density-gradient normals on the MI355X (include/hnrf_normals.h, csrc/hnrf_normals.hip): the three kernels against
their numpy twins (humannerf_amd/geometry.py) BIT FOR BIT, in guarded buffers under both fills; the gradient pass
(ops.density_gradient) against fp64 autograd with the kernels' own sign patterns; Network.ray_normals, the panels of
render_frames, Network.vertex_normals and the two exports end to end.  The twins themselves are held against float64
restatements in tests/test_normals_refs.py (no GPU)."""
import os

import numpy as np
import pytest
import torch

import guarded_buffers as gb
import normals_cases as nc
from humannerf_amd import geometry as geo
from tests import gltf_walker as walker

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EPS = nc.EPS_CANONICAL


def T(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def same(a, b):
    """Bit for bit; a NaN equals a NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def _lib():
    from humannerf_amd import _lib as L
    return L, L.load_normals()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _under_both_fills(call, outputs):
    """``call(fill)`` -> {name: GuardedBuffer}, every input and output guarded; the guards hold, and the ``outputs``
    hold the same bits under both fills.  Returns the buffers of the first fill."""
    runs = [call(f) for f in gb.FILLS]
    torch.cuda.synchronize()
    for bufs in runs:
        for b in bufs.values():
            b.check()
    for k in outputs:
        gb.same_bits(runs[0][k], runs[1][k])
    return runs[0]


# ------------------------------------------------------------------------------------------------- hnrf_ray_normals
def _ray_call(case, fill, alpha_min=0.5):
    L, lib = _lib()
    w, bmw, Rs, idx, g, alpha = case
    R, S = w.shape
    b = {k: gb.place(T(v), fill, name=k) for k, v in dict(weights=w, bmw=bmw, motion_Rs=Rs, idx=idx, g=g, alpha=alpha,
                                                         count=np.array([idx.size], np.int32)).items()}
    b['workspace'] = gb.GuardedBuffer(lib.hnrf_ray_normals_workspace_bytes(R, S), fill, DEV, 'workspace')
    b['normal'] = gb.GuardedBuffer(R * 12, fill, DEV, 'normal')
    b['nvalid'] = gb.GuardedBuffer(R, fill, DEV, 'nvalid')
    L.check(lib.hnrf_ray_normals(b['weights'].ptr, b['bmw'].ptr, b['motion_Rs'].ptr, b['idx'].ptr, b['count'].ptr, idx.size,
                                 b['g'].ptr, b['alpha'].ptr, R, S, bmw.shape[2], alpha_min, b['workspace'].ptr,
                                 b['workspace'].nbytes, b['normal'].ptr, b['nvalid'].ptr, _stream()), 'hnrf_ray_normals')
    return b


@pytest.mark.parametrize('S', nc.S_LIST)
@pytest.mark.parametrize('R', [1, 3, 65])
def test_ray_normals_equal_twin(R, S):
    """R around the four rays of a workgroup and many workgroups; S at the lane-stride edges; kept sets none / one / all
    and the mixed rows (a NaN weight, zero gradients, NaN and small alphas); B = 24 and B = 5."""
    for kept, B in (('mixed', 24), ('none', 24), ('one', 5), ('all', 24)):
        case = nc.ray_case(R, S, B, seed=1000 * R + S + B, kept=kept)
        want_n, want_ok = geo.ray_normals_host(*case)
        b = _under_both_fills(lambda fill: _ray_call(case, fill), ['normal', 'nvalid'])
        assert same(b['normal'].view(torch.float32, R, 3).cpu().numpy(), want_n), (kept, B)
        assert same(b['nvalid'].view(torch.uint8).cpu().numpy(), want_ok), (kept, B)
        if kept == 'none':
            assert not want_ok.any()
        if kept == 'all' and R > 1:
            assert want_ok.any()


def test_ray_normals_through_ops_and_compaction():
    """ops.ray_normals fed by ops.compact_samples: the kept set of the device is the twin's (w >= weight_min, a NaN is
    not kept) in the order the compaction's blocks arrived in -- which does not matter: row k of g belongs to idx[k];
    a count beyond the rows of g is read as the rows of g."""
    from humannerf_amd import ops
    w, bmw, Rs, idx, g, alpha = nc.ray_case(7, 65, 24, seed=9)
    didx, dcount = ops.compact_samples(T(w), nc.WEIGHT_MIN)
    order = didx[:idx.size].cpu().numpy()
    assert int(dcount) == idx.size and np.array_equal(np.sort(order), idx)
    g_dev = g[np.searchsorted(idx, order)]                                     # the case's gradients, in the device's order
    want_n, want_ok = geo.ray_normals_host(w, bmw, Rs, idx, g, alpha)
    assert same(geo.ray_normals_host(w, bmw, Rs, order, g_dev, alpha)[0], want_n)
    n, ok = ops.ray_normals(T(w), T(bmw), T(Rs), didx, dcount, T(g_dev), T(alpha))
    assert same(n.cpu().numpy(), want_n) and same(ok.cpu().numpy(), want_ok)
    half = idx.size // 2
    n, ok = ops.ray_normals(T(w), T(bmw), T(Rs), didx, dcount, T(g_dev[:half]), T(alpha))
    want_n, want_ok = geo.ray_normals_host(w, bmw, Rs, order[:half], g_dev[:half], alpha)
    assert same(n.cpu().numpy(), want_n) and same(ok.cpu().numpy(), want_ok)


def test_ray_normals_refusals():
    """Non-zero before any launch, the message names the argument, and the outputs keep their fill."""
    L, lib = _lib()
    case = nc.ray_case(3, 4, 24, seed=1, kept='all')
    w, bmw, Rs, idx, g, alpha = case
    b = _ray_call(case, gb.FILLS[0])
    torch.cuda.synchronize()
    out_n, out_v = gb.GuardedBuffer(36, gb.FILLS[0], DEV, 'normal'), gb.GuardedBuffer(3, gb.FILLS[0], DEV, 'nvalid')
    ws = b['workspace']
    bad_ws = gb.GuardedBuffer(ws.nbytes, gb.FILLS[0], DEV, 'workspace')
    odd = gb.GuardedBuffer(ws.nbytes + 4, gb.FILLS[0], DEV, 'workspace')

    def call(S=4, B=24, R=3, wsp=ws.ptr, wsb=ws.nbytes, weights=b['weights'].ptr, normal=out_n.ptr, amin=0.5, n_max=idx.size):
        return lib.hnrf_ray_normals(weights, b['bmw'].ptr, b['motion_Rs'].ptr, b['idx'].ptr, b['count'].ptr, n_max, b['g'].ptr,
                                    b['alpha'].ptr, R, S, B, amin, wsp, wsb, normal, out_v.ptr, _stream())
    for kw, word in ((dict(S=0), 'S 0'), (dict(S=513), 'S 513'), (dict(B=33), 'B 33'), (dict(B=0), 'B 0'), (dict(R=-1), 'R -1'),
                     (dict(weights=0), 'null'), (dict(normal=0), 'null'), (dict(wsp=0), 'workspace'),
                     (dict(wsp=odd.ptr + 2), 'aligned'), (dict(wsb=ws.nbytes - 4), 'workspace'),
                     (dict(amin=float('nan')), 'alpha_min'), (dict(n_max=-1), 'n_max')):
        assert call(**kw) != 0, kw
        assert word in lib.hnrf_last_error().decode(), (kw, lib.hnrf_last_error())
    # the workspace rule of include/hnrf.h: 256-byte aligned (HNRF_E_ARG = -1), a short one is HNRF_E_WORKSPACE = -4
    for kw, code, word in ((dict(wsp=odd.ptr + 4), -1, '256-byte aligned'), (dict(wsp=odd.ptr + 2), -1, '256-byte aligned'),
                           (dict(wsb=ws.nbytes - 1), -4, 'workspace'), (dict(wsb=ws.nbytes - 4), -4, 'workspace'),
                           (dict(wsb=0), -4, 'workspace')):
        assert call(**kw) == code, kw
        assert word in lib.hnrf_last_error().decode(), (kw, lib.hnrf_last_error())
    torch.cuda.synchronize()
    out_n.holds_fill(), out_v.holds_fill(), bad_ws.holds_fill()
    assert lib.hnrf_ray_normals_workspace_bytes(3, 0) == 0 and lib.hnrf_ray_normals_workspace_bytes(3, 513) == 0
    assert lib.hnrf_ray_normals_workspace_bytes(0, 4) == 0 and lib.hnrf_ray_normals_workspace_bytes(3, 4) == 48
    assert call(R=0) == 0                                                      # nothing launched, nothing written
    torch.cuda.synchronize()
    out_n.holds_fill()


# ----------------------------------------------------------------------------------------------- hnrf_normal_panels
def _panel_call(c, p2r, H, W, fill, surface, status_value=0):
    L, lib = _lib()
    b = {k: gb.place(T(c[k]), fill, name=k) for k in ('rays_d', 'normal', 'nvalid', 'valid', 'alpha', 'M', 'bgcolor')}
    b['pix2ray'] = gb.place(T(p2r.astype(np.int32)), fill, name='pix2ray')
    b['status'] = gb.place(T(np.array([status_value], np.int32)), fill, name='status')
    for k, n in (('o_normal', H * W * 12), ('o_nvalid', H * W), ('o_normal8', H * W * 3), ('o_shaded8', H * W * 3)):
        b[k] = gb.GuardedBuffer(n, fill, DEV, k)
    L.check(lib.hnrf_normal_panels(b['rays_d'].ptr, b['normal'].ptr, b['nvalid'].ptr, b['valid'].ptr, surface, b['alpha'].ptr,
                                   b['pix2ray'].ptr, c['N'], H, W, b['M'].ptr, b['bgcolor'].ptr, 0.25, 0.8, b['status'].ptr,
                                   b['o_normal'].ptr, b['o_nvalid'].ptr, b['o_normal8'].ptr, b['o_shaded8'].ptr, _stream()),
            'hnrf_normal_panels')
    return b


@pytest.mark.parametrize('H,W', [(1, 1), (5, 7), (16, 16)])
def test_normal_panels_equal_twin(H, W):
    """Two rays on one pixel, pixels without a ray, rays without a normal or a surface; both surfaces; through the
    device's own hnrf_pixel_rays; nothing is written under a raised status word."""
    from humannerf_amd import ops
    outs = ['o_normal', 'o_nvalid', 'o_normal8', 'o_shaded8']
    for surface in (0, 1):
        c = nc.panel_case(H, W, seed=H * W + surface)
        p2r, st = geo.pixel_rays_host(c['ray_index'], H, W)
        dp2r, dst = ops.pixel_rays(T(c['ray_index']), H, W)
        assert st == 0 and int(dst) == 0 and np.array_equal(dp2r.cpu().numpy(), p2r)
        want = geo.normal_panels_host(c['rays_d'], c['normal'], c['nvalid'], c['valid'], p2r, H, W, surface=surface,
                                      alpha=c['alpha'], M=c['M'], bgcolor=c['bgcolor'])
        b = _under_both_fills(lambda fill: _panel_call(c, p2r, H, W, fill, surface), outs)
        assert same(b['o_normal'].view(torch.float32, H, W, 3).cpu().numpy(), want['normal'])
        assert same(b['o_nvalid'].view(torch.uint8, H, W).cpu().numpy(), want['nvalid'])
        assert same(b['o_normal8'].view(torch.uint8, H, W, 3).cpu().numpy(), want['normal8'])
        assert same(b['o_shaded8'].view(torch.uint8, H, W, 3).cpu().numpy(), want['shaded8'])
        got = ops.normal_panels(T(c['rays_d']), T(c['normal']), T(c['nvalid']), T(c['valid']), dp2r, H, W,
                                ['normal8', 'shaded8'], surface=surface, alpha=T(c['alpha']), M=T(c['M']), bgcolor=T(c['bgcolor']),
                                status=dst)
        assert sorted(got) == ['normal8', 'shaded8'] and all(same(got[k].cpu().numpy(), want[k]) for k in got)
    raised = _panel_call(c, p2r, H, W, gb.FILLS[0], 0, status_value=1)
    torch.cuda.synchronize()
    for k in outs:
        raised[k].holds_fill()


def test_normal_panels_refusals():
    L, lib = _lib()
    c = nc.panel_case(2, 2, seed=1)
    p2r, _ = geo.pixel_rays_host(c['ray_index'], 2, 2)
    b = _panel_call(c, p2r, 2, 2, gb.FILLS[0], 0)
    torch.cuda.synchronize()
    out = gb.GuardedBuffer(12, gb.FILLS[0], DEV, 'normal8')

    def call(H=2, W=2, N=c['N'], surface=0, M=b['M'].ptr, alpha=b['alpha'].ptr, p=b['pix2ray'].ptr, n8=out.ptr, s8=0, amb=0.25):
        return lib.hnrf_normal_panels(b['rays_d'].ptr, b['normal'].ptr, b['nvalid'].ptr, b['valid'].ptr, surface, alpha, p, N, H,
                                      W, M, b['bgcolor'].ptr, amb, 0.8, 0, 0, 0, n8, s8, _stream())
    for kw, word in ((dict(H=0), 'H 0'), (dict(W=16385), 'W 16385'), (dict(N=-1), 'N -1'), (dict(surface=2), 'surface'),
                     (dict(M=0), 'normal8 needs M'), (dict(alpha=0, n8=0, s8=out.ptr), 'shaded8 needs alpha'),
                     (dict(p=0), 'null'), (dict(p=b['pix2ray'].ptr + 2), 'aligned'), (dict(amb=float('nan')), 'NaN')):
        assert call(**kw) != 0, kw
        assert word in lib.hnrf_last_error().decode(), (kw, lib.hnrf_last_error())
    torch.cuda.synchronize()
    out.holds_fill()


# ----------------------------------------------------------------------------------------------- hnrf_field_normals
def _field_call(case, fill, B):
    L, lib = _lib()
    verts, g, sigma, vol, bmin, scale = case
    b = {k: gb.place(T(v), fill, name=k) for k, v in dict(verts=verts, g=g, sigma=sigma, vol=vol, bmin=bmin, scale=scale).items()}
    b['normal'] = gb.GuardedBuffer(len(verts) * 12, fill, DEV, 'normal')
    L.check(lib.hnrf_field_normals(b['verts'].ptr, b['g'].ptr, b['sigma'].ptr, len(verts), b['vol'].ptr, B, vol.shape[-1],
                                   b['bmin'].ptr, b['scale'].ptr, b['normal'].ptr, _stream()), 'hnrf_field_normals')
    return b


@pytest.mark.parametrize('V', [0, 1, 77, 300])
def test_field_normals_equal_twin(V):
    """No vertex, one, a ragged workgroup and more than one workgroup; vertices inside the volume and in the zero-padded
    shell, densities of both signs, a zero gradient; unit length within 2^-22 where not zero."""
    case = nc.field_case(V, 24, 8, seed=V)
    want = geo.field_normals_host(*case, n_bones=24)
    b = _under_both_fills(lambda fill: _field_call(case, fill, 24), ['normal'])
    got = b['normal'].view(torch.float32, V, 3).cpu().numpy()
    assert same(got, want)
    lens = np.linalg.norm(got.astype(np.float64), axis=1)
    assert ((lens == 0) | (np.abs(lens - 1) <= 2.0 ** -22)).all()
    if V >= 77:
        assert (lens > 0).sum() > V // 4 and (lens == 0).any()


def test_field_normals_refusals():
    L, lib = _lib()
    case = nc.field_case(5, 24, 8, seed=1)
    b = _field_call(case, gb.FILLS[0], 24)
    torch.cuda.synchronize()
    out = gb.GuardedBuffer(60, gb.FILLS[0], DEV, 'normal')

    def call(V=5, B=24, G=8, verts=b['verts'].ptr, normal=out.ptr):
        return lib.hnrf_field_normals(verts, b['g'].ptr, b['sigma'].ptr, V, b['vol'].ptr, B, G, b['bmin'].ptr, b['scale'].ptr,
                                      normal, _stream())
    for kw, word in ((dict(V=-1), 'V -1'), (dict(B=0), 'B 0'), (dict(B=33), 'B 33'), (dict(G=1), 'G 1'), (dict(G=1025), 'G 1025'),
                     (dict(verts=0), 'null'), (dict(normal=0), 'null')):
        assert call(**kw) != 0, kw
        assert word in lib.hnrf_last_error().decode(), (kw, lib.hnrf_last_error())
    assert call(V=0, verts=0, normal=0) == 0
    torch.cuda.synchronize()
    out.holds_fill()


# ------------------------------------------------------------------------------------------------- the gradient pass
def _problem(P, seed):
    """Both MLPs' weights of one seeded state ('scaled' regime: offsets of a few cm), skeleton points, condition code and
    window of tests/test_train_kernel_refs.py::make_problem."""
    from tests.test_train_kernel_refs import SPECS, make_problem
    nr = make_problem('nonrigid', P, seed, regime='scaled')
    cn = dict(kind='canonical', P=P, st=nr['st'], ws=[nr['st'][n + '.weight'] for n in SPECS['canonical']['names']],
              bs=[nr['st'][n + '.bias'] for n in SPECS['canonical']['names']])
    return nr, cn


def _masks(acts, P):
    return [(acts[l, :P] > 0).double().cpu() for l in range(acts.shape[0])]


def _gradient_reference(nr, cn, mode, with_warp, x):
    """fp64 autograd of sigma with respect to ``x`` (P, 3) fp32 -- canonical points, or with ``with_warp`` skeleton
    points, through xyz = x + offset(x) -- with the ReLU sign patterns of the device's own forward (taken from the code
    under test, as tests/test_gpu_train_kernels.py does).  With ``with_warp`` the canonical gradient is taken AT THE
    DEVICE'S xyz, which is what the pass is defined by (xyz comes from hnrf_nonrigid_fwd_train) and what the bound
    'two chained kernels, each within eps' is about: each backward kernel against fp64 on the inputs it was given.  At
    the fp64 xyz instead, the rounding of the forward's xyz (1e-7 .. 1e-6) times the second derivative of a field
    with frequencies up to 2^9 moves the gradient by 4e-5 .. 9e-5 of its largest element (measured), which is no error
    of either chain.  Returns (g_ref (P, 3) float64, the points the canonical MLP was evaluated at)."""
    from humannerf_amd import ops
    from tests.test_train_kernel_refs import ref_mlp, ref_mlp_grads
    P = x.shape[0]
    cws, cbs = [T(w) for w in cn['ws']], [T(b) for b in cn['bs']]
    cpk = ops.canonical_pack(cws, cbs, mode)
    one = np.zeros((P, 4), np.float32)
    one[:, 3] = 1
    if not with_warp:
        acts = ops.canonical_train(T(x), cpk, mode)[2]
        return ref_mlp_grads(dict(cn, x=x), _masks(acts, P), one)['d_x'].numpy(), x
    npk = ops.nonrigid_pack([T(w) for w in nr['ws']], [T(b) for b in nr['bs']], T(nr['cond']), mode)
    xyz_dev, _, _, nacts, _ = ops.nonrigid_train(T(x), T(nr['hann']), npk, mode)
    nmasks = _masks(nacts, P)
    cmasks = _masks(ops.canonical_train(xyz_dev, cpk, mode)[2], P)
    xyz = xyz_dev.cpu().numpy().reshape(P, 3)
    xyz64 = ref_mlp(dict(nr, x=x), nmasks)['out'].detach().numpy()                      # the forward itself: 1e-5 of fp64
    assert np.abs(xyz - xyz64).max() <= 1e-5 * max(1.0, np.abs(xyz64).max())
    d_xyz = ref_mlp_grads(dict(cn, x=xyz), cmasks, one)['d_x'].numpy()
    return ref_mlp_grads(dict(nr, x=x), nmasks, d_xyz)['d_x'].numpy(), xyz


def _gradient_bounds(got, ref, eps, label):
    """Each component within eps max|ref element|; the unit normal within sqrt(3) eps max|ref element| / |g_ref| radians
    (a vector whose three components are each off by at most e is off by at most sqrt(3) e in length, seen from its tip
    under at most that over its length).  Samples whose |g_ref| is below 1 % of the case's largest are left out of the
    angle, at most 5 % of them."""
    top = np.abs(ref).max()
    err = np.abs(got.astype(np.float64) - ref).max()
    norm = np.linalg.norm(ref, axis=1)
    keep = norm >= 0.01 * norm.max()
    ang = nc.angle(got[keep] / np.linalg.norm(got[keep].astype(np.float64), axis=1, keepdims=True), ref[keep] / norm[keep, None])
    lim = np.sqrt(3) * eps * top / norm[keep]
    print('%s: component error %.2e of the largest element (bound %.0e); worst angle %.2e rad, %.2f of its bound; left out %d'
          % (label, err / top, eps, ang.max(), (ang / lim).max(), (~keep).sum()))
    assert err <= eps * top, (label, err / top)
    assert (~keep).mean() <= 0.05, label
    assert (ang <= lim).all(), (label, float((ang / lim).max()))


@pytest.mark.parametrize('P', [1, 127, 129, 1000])
@pytest.mark.parametrize('with_warp', [False, True], ids=['canonical', 'warp'])
@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
def test_density_gradient_against_fp64(mode, with_warp, P):
    """ops.density_gradient against fp64: eps = 2e-5 for the canonical chain alone (the bound
    tests/test_gpu_train_kernels.py holds d_x to), twice that with the non-rigid chain behind it (two chained kernels,
    each within eps).  sigma is the forward's.  Chunks of 128 give the bits of one chunk, and the backward images may be
    given packed or as weights."""
    from humannerf_amd import ops
    from tests.test_train_kernel_refs import ref_mlp
    nr, cn = _problem(P, 11 + P % 3)
    x = nr['x'] if with_warp else np.random.RandomState(P).uniform(-1.2, 1.2, (P, 3)).astype(np.float32)
    cws, cbs = [T(w) for w in cn['ws']], [T(b) for b in cn['bs']]
    cpk = ops.canonical_pack(cws, cbs, mode)
    warp = None
    if with_warp:
        nws = [T(w) for w in nr['ws']]
        npk = ops.nonrigid_pack(nws, [T(b) for b in nr['bs']], T(nr['cond']), mode)
        warp = (T(x), T(nr['hann']), npk, nws)
    g, sigma = ops.density_gradient(None if with_warp else T(x), cpk, cws, mode, warp=warp)
    assert g.shape == (P, 3) and sigma.shape == (P,)
    ref, xyz = _gradient_reference(nr, cn, mode, with_warp, x)
    _gradient_bounds(g.cpu().numpy(), ref, 2 * EPS if with_warp else EPS, 'density_gradient %s %s P=%d' % (mode, 'warp' if with_warp else 'canonical', P))
    s64 = ref_mlp(dict(cn, x=xyz))['out'][:, 3].detach().numpy()
    assert np.abs(sigma.cpu().numpy() - s64).max() <= 1e-4 * max(1.0, np.abs(s64).max())
    # chunking, a kept workspace used twice, and packed backward images
    ws = {}
    packed = (ops.canonical_bwd_pack(cws, mode),)
    if with_warp:
        warp = warp[:3] + (ops.nonrigid_bwd_pack(nws, mode),)
    for _ in range(2):
        g2, s2 = ops.density_gradient(None if with_warp else T(x), cpk, packed[0], mode, warp=warp, workspace=ws, chunk=128)
        assert torch.equal(g2.view(torch.int32), g.view(torch.int32)) and torch.equal(s2.view(torch.int32), sigma.view(torch.int32))
    assert ws['key'][0] == 128


def test_density_gradient_workspace_bytes_are_as_documented():
    from humannerf_amd import ops
    ws = ops._gradient_workspace({}, 256, True, DEV)
    cn = sum(ws[k].numel() * ws[k].element_size() for k in ('raw', 'pe', 'acts', 'bits', 'dZ', 'd_raw'))
    nr = sum(ws[k].numel() * ws[k].element_size() for k in ws if k.startswith('nr_'))
    assert cn == 256 * ops.GRADIENT_BYTES_CANONICAL and nr == 256 * ops.GRADIENT_BYTES_NONRIGID
    g, s = ops.density_gradient(torch.zeros(0, 3, device=DEV), torch.zeros(4, device=DEV), [], 'f32')
    assert g.shape == (0, 3) and s.shape == (0,)


# --------------------------------------------------------------------------------- the network, the loops, the files
def _seeded_net():
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state, with_density
    n = Network()
    n.load_state_dict({k: torch.from_numpy(v) for k, v in with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0).items()})
    return n.to(DEV).eval()


@pytest.fixture(scope='module')
def net():
    return _seeded_net()


@pytest.fixture(scope='module')
def subject(tmp_path_factory):
    from humannerf_amd import dataset, scene
    root = str(tmp_path_factory.mktemp('normals') / 'subject')
    names = scene.write_synthetic_subject(root, n_frames=3, size=16)
    return dataset.Subject(root), names


@pytest.fixture()
def loop_cfg():
    from humannerf_amd.config import cfg
    amd = cfg.amd
    keys = ('metrics', 'video', 'maps', 'maps_surface', 'maps_normals', 'normal_weight_min', 'canonical', 'bake_resolution',
            'diagnostics', 'mlp_mode')
    old = (cfg.get('show_truth', False), cfg.get('show_alpha', False), cfg.N_samples, cfg.ignore_non_rigid_motions, cfg.perturb,
           {k: amd[k] for k in keys if k in amd})
    cfg.N_samples, cfg.show_alpha, amd.diagnostics, cfg.perturb = 16, True, True, 0.
    yield cfg
    cfg.show_truth, cfg.show_alpha, cfg.N_samples, cfg.ignore_non_rigid_motions, cfg.perturb = old[:5]
    for k in keys:
        if k in old[5]:
            amd[k] = old[5][k]
        else:
            amd.pop(k, None)


def _frames(subject):
    from humannerf_amd import run
    return run._Frames(len(subject), lambda i: subject.movement_frame(i, load_image=True, device=DEV))


def _render(net, subject, monkeypatch, maps):
    """render_frames over the subject's frames -> (panels {idx: {name: array}}, the inputs of every geometry.frame_maps
    call with the device tensors it was given)."""
    from humannerf_amd import render
    calls, panels = [], {}
    real = geo.frame_maps

    def spy(data, out, H, W, ray_index, **kw):
        calls.append(dict(data=data, out={k: v.clone() for k, v in out.items()}, H=H, W=W, ray_index=ray_index.clone(),
                          kw={k: (tuple(t.clone() for t in v) if k == 'ray_normals' else v) for k, v in kw.items()}))
        return real(data, out, H, W, ray_index, **kw)

    monkeypatch.setattr(geo, 'frame_maps', spy)
    render.render_frames(net, _frames(subject), device=DEV, show_truth=True, maps=maps,
                         on_maps=lambda i, p: panels.__setitem__(i, {k: v.copy() for k, v in p.items()}))
    monkeypatch.setattr(geo, 'frame_maps', real)
    return panels, calls


def _frame_inputs(net, subject, monkeypatch):
    """(data, out) of frame 1 as render_frames hands them to the network and gets them back."""
    _, calls = _render(net, subject, monkeypatch, ['depth'])
    assert len(calls) == 3 and calls[1]['H'] == calls[1]['W'] == 16
    return calls[1]['data'], calls[1]['out']


def _host(t):
    return t.detach().cpu().numpy()


def _twin_of_parts(data, out, parts, net, alpha_min=0.5):
    """ray_normals_host on the frame's outputs, the device's kept list and the device's gradients."""
    from humannerf_amd.network import motion_basis
    S = out['weights_on_rays'].shape[-1]
    w = _host(out['weights_on_rays']).reshape(-1, S)
    n = parts['n']
    with torch.no_grad():
        rvec = net.pose_decoder.rvec(data['dst_posevec'].float()[None]) if net._refines_pose(1e7) else None
        Rs, _ = motion_basis(data['dst_Rs'].float(), data['dst_Ts'].float(), data['cnl_gtfms'].float(), rvec)
    return geo.ray_normals_host(w, _host(out['backward_motion_weights']).reshape(w.shape[0], S, -1), _host(Rs),
                                _host(parts['idx'])[:n], _host(parts['g']), _host(out['alpha']).reshape(-1), alpha_min), _host(Rs)


def _fp64_ray_normals(net, data, out, parts, Rs, mode):
    """The same definition in float64 from the device's own skeleton points: grad through both MLPs by fp64 autograd
    (_gradient_reference), then nc.ray_normals_fp64; also the per-ray angle bound.  A unit normal of a sample is within
    theta_s = sqrt(3) eps' max|g_ref| / |g_ref,s| of its reference (the bound of the gradient pass), so N = sum w_s u_s is
    off by at most sum w_s theta_s and N / |N| by at most that over |N_ref|; 1e-6 is added for the fp32 sums of the
    kernel, which the twin test pins bit for bit."""
    from humannerf_amd.config import cfg
    from humannerf_amd.network import hann_window_weights
    from tests.test_train_kernel_refs import SPECS
    st = {k: _host(v) for k, v in net.state_dict().items()}
    nrc = cfg.non_rigid_motion_mlp
    chain = parts['chain']
    nr = dict(kind='nonrigid', ws=[st[n + '.weight'] for n in SPECS['nonrigid']['names']],
              bs=[st[n + '.bias'] for n in SPECS['nonrigid']['names']], cond=_host(data['dst_posevec']).reshape(-1).astype(np.float32),
              hann=hann_window_weights(1e7, nrc.multires, nrc.kick_in_iter, nrc.full_band_iter).numpy().astype(np.float32))
    cn = dict(kind='canonical', ws=[st[n + '.weight'] for n in SPECS['canonical']['names']],
              bs=[st[n + '.bias'] for n in SPECS['canonical']['names']])
    x = _host(parts['x'])
    ref, _ = _gradient_reference(nr, cn, mode, chain, x)
    S = out['weights_on_rays'].shape[-1]
    w = _host(out['weights_on_rays']).reshape(-1, S)
    idx = _host(parts['idx'])[:parts['n']]
    n64, ok64 = nc.ray_normals_fp64(w, _host(out['backward_motion_weights']).reshape(w.shape[0], S, -1), Rs, idx, ref,
                                    _host(out['alpha']).reshape(-1))
    eps = 2 * EPS if chain else EPS
    norm = np.linalg.norm(ref, axis=1)
    small = norm < 0.01 * norm.max()
    theta = np.sqrt(3) * eps * np.abs(ref).max() / np.maximum(norm, 1e-300)
    m64 = _host(out['backward_motion_weights']).reshape(-1, Rs.shape[0]).astype(np.float64)
    num, N = np.zeros(w.shape[0]), np.zeros((w.shape[0], 3))
    left_out = np.zeros(w.shape[0], bool)
    for k, p in enumerate(idx):
        num[p // S] += float(w.reshape(-1)[p]) * theta[k]
        left_out[p // S] |= small[k]
        A = np.einsum('b,bij->ij', m64[p], Rs.astype(np.float64))
        v = -(A.T @ ref[k])
        N[p // S] += float(w.reshape(-1)[p]) * v / np.linalg.norm(v)
    bound = num / np.maximum(np.linalg.norm(N, axis=1), 1e-300) + 1e-6
    return n64, ok64, bound, left_out, ref


def _check_frame(net, data, out, mode, label):
    normal, nvalid, parts = net.ray_normals(data, out, want_parts=True)
    (tw_n, tw_ok), Rs = _twin_of_parts(data, out, parts, net)
    assert same(_host(normal), tw_n) and same(_host(nvalid), tw_ok), label
    n64, ok64, bound, left_out, ref = _fp64_ray_normals(net, data, out, parts, Rs, mode)
    assert np.array_equal(tw_ok.astype(bool), ok64), label
    use = ok64 & ~left_out
    assert use.any() and left_out[ok64].mean() <= 0.05, (label, use.sum(), left_out[ok64].mean())
    ang = nc.angle(_host(normal)[use], n64[use])
    print('%s: %d kept samples, %d valid rays, worst angle %.2e rad, %.2f of its bound'
          % (label, parts['n'], ok64.sum(), ang.max(), (ang / bound[use]).max()))
    assert (ang <= bound[use]).all(), (label, float((ang / bound[use]).max()))
    return normal, nvalid, parts


def test_network_ray_normals_on_a_small_frame(net, subject, loop_cfg, monkeypatch):
    """16 x 16 pixels, S = 16, the seeded network: Network.ray_normals equals the twin fed with the device's gradients bit
    for bit and the all-fp64 evaluation within the derived angle bound; the same holds for a frame rendered with
    cfg.amd.canonical = 'baked' (the MLPs are evaluated all the same); a second call of a long-lived Network returns the
    same bits from its kept backward images, and weights_changed() after a change of the canonical weights rebuilds
    them; with cfg.ignore_non_rigid_motions the result is the warp-free path on xyz_on_rays."""
    from humannerf_amd import ops, run
    sub, _ = subject
    net.weights_changed()
    mode = net._mlp_mode()
    data, out = _frame_inputs(net, sub, monkeypatch)
    normal, nvalid, parts = _check_frame(net, data, out, mode, 'exact')
    assert parts['chain'] and bool(nvalid.any())
    packs = {k: e.packed.data_ptr() for k, e in net._kept.items() if k[0] == 'pack_bwd'}
    assert sorted(k[1] for k in packs) == ['canonical', 'nonrigid']
    again, again_ok = net.ray_normals(data, out)
    assert torch.equal(again.view(torch.int32), normal.view(torch.int32)) and torch.equal(again_ok, nvalid)
    assert {k: e.packed.data_ptr() for k, e in net._kept.items() if k[0] == 'pack_bwd'} == packs      # kept, not re-packed
    serial = net._pack_serial
    net.ray_normals(data, out)
    assert net._pack_serial == serial
    # changed canonical weights, through .data: invisible until weights_changed()
    head = net.cnl_mlp.module.linears()[3].weight
    saved = head.data.clone()
    try:
        head.data.mul_(1.5)
        stale, _ = net.ray_normals(data, out)
        assert torch.equal(stale.view(torch.int32), normal.view(torch.int32))
        net.weights_changed()
        fresh, _ = net.ray_normals(data, out)
        assert not torch.equal(fresh.view(torch.int32), normal.view(torch.int32))
    finally:
        head.data.copy_(saved)
        net.weights_changed()
    back, _ = net.ray_normals(data, out)
    assert torch.equal(back.view(torch.int32), normal.view(torch.int32))
    # baked canonical grid: other weights on the rays, the same checks
    loop_cfg.amd.canonical, loop_cfg.amd.bake_resolution = 'baked', 32
    run._baked_folder(net, sub, 'movement')
    bdata, bout = _frame_inputs(net, sub, monkeypatch)
    _check_frame(net, bdata, bout, mode, 'baked')
    loop_cfg.amd.canonical = 'mlp'
    # no non-rigid motion: the gradient at xyz_on_rays, no chain
    loop_cfg.ignore_non_rigid_motions = True
    idata, iout = _frame_inputs(net, sub, monkeypatch)
    n_i, ok_i, p_i = net.ray_normals(idata, iout, want_parts=True)
    assert not p_i['chain']
    kept = p_i['idx'][:p_i['n']].long()
    g_direct, _ = net.density_gradient(iout['xyz_on_rays'].reshape(-1, 3)[kept])
    assert torch.equal(g_direct.view(torch.int32), p_i['g'].view(torch.int32))
    (tw_n, tw_ok), _ = _twin_of_parts(idata, iout, p_i, net)
    assert same(_host(n_i), tw_n) and same(_host(ok_i), tw_ok)
    loop_cfg.ignore_non_rigid_motions = False
    with pytest.raises(ValueError, match='diagnostics'):
        net.ray_normals(data, {k: out[k] for k in ('rgb', 'alpha', 'depth')})


def test_network_density_gradient_with_a_frame(net, subject, loop_cfg):
    """Network.density_gradient: canonical points against ops.density_gradient on the network's own images; with a frame
    the non-rigid chain is included (another result), and with cfg.ignore_non_rigid_motions it is not."""
    from humannerf_amd import ops
    sub, _ = subject
    pts = torch.from_numpy(np.random.RandomState(0).uniform(-0.5, 0.5, (129, 3)).astype(np.float32)).to(DEV)
    g, s = net.density_gradient(pts)
    lin = net.cnl_mlp.module.linears()
    g2, s2 = ops.density_gradient(pts, net._canonical_packed(), [l.weight.detach() for l in lin], net._mlp_mode())
    assert torch.equal(g.view(torch.int32), g2.view(torch.int32)) and torch.equal(s.view(torch.int32), s2.view(torch.int32))
    frame = sub.movement_frame(1, image_size=(1, 1))
    gf, _ = net.density_gradient(pts, frame)
    assert gf.shape == (129, 3) and bool(torch.isfinite(gf).all()) and not torch.equal(gf, g)
    loop_cfg.ignore_non_rigid_motions = True
    gi, _ = net.density_gradient(pts, frame)
    assert torch.equal(gi.view(torch.int32), g.view(torch.int32))


def test_render_frames_with_gradient_normals(net, subject, loop_cfg, monkeypatch):
    """maps_normals = 'gradient': the normal and shaded panels equal normal_panels_host on the device's ray normals, the
    depth panel is the screen path's; 'screen' delivers the bytes it delivers when the option is left out."""
    from humannerf_amd import render
    sub, _ = subject
    maps = ['depth', 'normal', 'shaded']
    loop_cfg.amd.pop('maps_normals', None)
    plain, calls0 = _render(net, sub, monkeypatch, maps)
    assert all('ray_normals' not in c['kw'] for c in calls0)
    loop_cfg.amd.maps_normals = 'screen'
    screen, _ = _render(net, sub, monkeypatch, maps)
    assert sorted(screen) == sorted(plain) == [0, 1, 2]
    assert all(screen[i][m].tobytes() == plain[i][m].tobytes() for i in plain for m in maps)
    loop_cfg.amd.maps_normals = 'gradient'
    grad, calls = _render(net, sub, monkeypatch, maps)
    assert sorted(grad) == [0, 1, 2] and len(calls) == 3
    differs = False
    for i, c in enumerate(calls):
        rn, rv = (_host(t) for t in c['kw']['ray_normals'])
        d, o = c['data'], c['out']
        surf = geo.ray_surface_host(_host(d['near']), _host(d['far']), _host(o['alpha']), _host(o['depth']))
        p2r, st = geo.pixel_rays_host(_host(c['ray_index']), c['H'], c['W'])
        M = c['kw']['M'] if c['kw'].get('M') is not None else np.eye(3)
        M = _host(M) if torch.is_tensor(M) else M
        want = geo.normal_panels_host(_host(d['rays'][1]), rn, rv, surf['valid'], p2r, c['H'], c['W'], want=['normal8', 'shaded8'],
                                      alpha=_host(o['alpha']), M=M, bgcolor=_host(d['bgcolor']).astype(np.float32) / np.float32(255.))
        assert st == 0 and list(grad[i]) == maps
        assert same(grad[i]['normal'], want['normal8']) and same(grad[i]['shaded'], want['shaded8']), i
        assert grad[i]['depth'].tobytes() == plain[i]['depth'].tobytes()
        differs |= grad[i]['normal'].tobytes() != plain[i]['normal'].tobytes()
        assert rv.any()
    assert differs
    loop_cfg.amd.diagnostics = False
    with pytest.raises(ValueError, match='diagnostics'):
        render.render_frames(net, _frames(sub), device=DEV, maps=maps)


LEVEL = 10.0           # with the sigma bias raised by 5 (with_density), as tests/test_gpu_mesh.py cuts the surface


def test_vertex_normals_equal_twin(net, subject):
    """Network.vertex_normals on the N = 32 mesh: hnrf_field_normals equals the twin on the device's g and sigma bit for
    bit, and every non-zero normal has unit length within 2^-22."""
    sub, _ = subject
    bbox = sub.canonical_bbox
    verts, faces, _ = net.extract_canonical_mesh(bbox['min_xyz'], bbox['max_xyz'], sub.motion_weights_priors, resolution=32, level=LEVEL)
    assert verts.shape[0] > 100
    n, g, sigma, vol = net.vertex_normals(verts, sub.motion_weights_priors, bbox['min_xyz'], bbox['max_xyz'], want_parts=True)
    bmin, _, scale = net._mesh_bbox(bbox['min_xyz'], bbox['max_xyz'])
    want = geo.field_normals_host(_host(verts), _host(g), _host(sigma), _host(vol), _host(bmin), _host(scale), vol.shape[0] - 1)
    assert same(_host(n), want)
    lens = np.linalg.norm(_host(n).astype(np.float64), axis=1)
    # (a vertex is an interpolated crossing of the lattice's density; where the field's own sigma is <= 0 there -- a
    # third of the vertices of this noise field at N = 32 -- D has no gradient and the normal is 0, as the header states)
    assert ((lens == 0) | (np.abs(lens - 1) <= 2.0 ** -22)).all() and (lens > 0).any()
    assert (lens[~(_host(sigma) > 0)] == 0).all()
    print('vertex normals at N = 32: %d vertices, %d with sigma <= 0 (normal 0)' % (len(lens), (lens == 0).sum()))
    assert net.vertex_normals(verts[:0], sub.motion_weights_priors, bbox['min_xyz'], bbox['max_xyz']).shape == (0, 3)


def test_run_mesh_and_run_gltf_with_normals(net, subject, tmp_path):
    """The files read back with V unit normals; the posed .ply has none; the glTF still re-poses every key-frame (gltf.pose
    and the independent walker), and normals=False writes the bytes of a call without the argument."""
    from humannerf_amd import gltf, mesh, run
    sub, names = subject
    out = run.run_mesh(net, sub, frames=(0,), resolution=32, level=LEVEL, logdir=str(tmp_path / 'm'), normals=True)
    v, f, c, n = mesh.read_ply(out['canonical'], want_normals=True)
    lens = np.linalg.norm(n.astype(np.float64), axis=1)
    assert n.shape == v.shape and len(v) > 100 and ((lens == 0) | (np.abs(lens - 1) <= 2.0 ** -22)).all() and (lens > 0).any()
    posed = [p for k, p in out.items() if k != 'canonical']
    assert len(posed) == 1 and mesh.read_ply(posed[0], want_normals=True)[3] is None
    plain = run.run_mesh(net, sub, resolution=32, level=LEVEL, logdir=str(tmp_path / 'p'))
    again = run.run_mesh(net, sub, resolution=32, level=LEVEL, logdir=str(tmp_path / 'q'), normals=False)
    assert open(plain['canonical'], 'rb').read() == open(again['canonical'], 'rb').read()
    assert np.array_equal(mesh.read_ply(plain['canonical'])[0], v)

    res = run.run_gltf(net, sub, resolution=32, level=LEVEL, logdir=str(tmp_path / 'g'), normals=True)
    ref = run.run_gltf(net, sub, resolution=32, level=LEVEL, logdir=str(tmp_path / 'h'))
    off = run.run_gltf(net, sub, resolution=32, level=LEVEL, logdir=str(tmp_path / 'i'), normals=False)
    assert open(ref['path'], 'rb').read() == open(off['path'], 'rb').read()
    glb, glb0 = gltf.read_glb(res['path']), gltf.read_glb(ref['path'])
    assert glb['normals'].shape == (res['V'], 3) and np.array_equal(glb['normals'], n) and 'normals' not in glb0
    doc, arr = walker.walk(res['path'])
    assert np.array_equal(arr[doc['meshes'][0]['primitives'][0]['attributes']['NORMAL']], n)
    for i in range(3):
        a = gltf.pose(glb, i, relative_to='global')
        assert np.abs(a - walker.posed(doc, arr, i)).max() <= 1e-9
        assert np.array_equal(a, gltf.pose(glb0, i, relative_to='global'))
