"""Density-gradient normals without a GPU: the numpy twins of include/hnrf_normals.h (humannerf_amd/geometry.py) against
independent float64 restatements (tests/normals_cases.py), the derivative of the gate against central differences, the
definition of the gradient against torch.autograd, the options, the file formats and the binding table."""
import numpy as np
import pytest
import torch

import normals_cases as nc
from humannerf_amd import geometry as geo


# ------------------------------------------------------------------------------------------------------ ray normals
@pytest.mark.parametrize('S', nc.S_LIST)
@pytest.mark.parametrize('kept', ['mixed', 'none', 'one', 'all'])
def test_ray_normals_twin_against_fp64(S, kept):
    """R = 9 rays of B = 24 bones: rays with no kept sample, one, all and a random half; zero gradients; a NaN alpha and
    alphas below alpha_min.  Validity agrees exactly, the unit normals within 1e-5 per component (fp32 sums of at most
    130 unit vectors against float64)."""
    w, bmw, Rs, idx, g, alpha = nc.ray_case(9, S, 24, seed=S + len(kept), kept=kept)
    n, ok = geo.ray_normals_host(w, bmw, Rs, idx, g, alpha)
    want, want_ok = nc.ray_normals_fp64(w, bmw, Rs, idx, g, alpha)
    assert n.dtype == np.float32 and n.shape == (9, 3) and ok.dtype == np.uint8
    assert np.array_equal(ok.astype(bool), want_ok)
    assert np.abs(n - want).max() <= 1e-5
    assert (n[ok == 0] == 0).all()
    if kept == 'none':
        assert not ok.any()
    if kept in ('one', 'all'):
        assert ok.sum() == (alpha >= 0.5).sum() or (g == 0).all(axis=1).any()
    lens = np.linalg.norm(n[ok == 1].astype(np.float64), axis=1)
    assert np.abs(lens - 1).max(initial=0) <= 2.0 ** -22


def test_ray_normals_twin_special_samples():
    """A kept sample with a NaN weight makes its ray invalid (normal 0) and no other; a zero gradient contributes
    nothing; one kept sample gives -A^T g / |A^T g| whatever its weight; the normal is not flipped."""
    w, bmw, Rs, idx, g, alpha = nc.ray_case(4, 65, 24, seed=3, kept='all')
    alpha[:] = 0.9
    g[2 * 65 + 64] = (30, -20, 10)                                            # (kept = all: row p of g is sample p)
    base, ok0 = geo.ray_normals_host(w, bmw, Rs, idx, g, alpha)
    assert ok0.all()
    wn = w.copy()
    wn[2, 64] = np.nan
    n, ok = geo.ray_normals_host(wn, bmw, Rs, idx, g, alpha)
    assert list(ok) == [1, 1, 0, 1] and (n[2] == 0).all() and np.array_equal(n[[0, 1, 3]], base[[0, 1, 3]])
    gz = g.copy()
    gz[65:130] = 0                                                            # every sample of ray 1
    n, ok = geo.ray_normals_host(w, bmw, Rs, idx, gz, alpha)
    assert list(ok) == [1, 0, 1, 1] and (n[1] == 0).all()
    one = np.array([70], np.int32)                                            # sample 5 of ray 1
    n, ok = geo.ray_normals_host(w, bmw, Rs, one, g[70:71], alpha)
    A = np.einsum('b,bij->ij', bmw[1, 5].astype(np.float64), Rs.astype(np.float64))
    v = -(A.T @ g[70].astype(np.float64))
    assert list(ok) == [0, 1, 0, 0] and np.abs(n[1] - v / np.linalg.norm(v)).max() <= 1e-6
    nf, _ = geo.ray_normals_host(w, bmw, Rs, one, -g[70:71], alpha)
    assert np.array_equal(nf[1], -n[1])                                       # the sign of the gradient is kept
    # an index outside the frame is skipped, and alpha_min is honoured
    n2, ok2 = geo.ray_normals_host(w, bmw, Rs, np.array([70, 4 * 65], np.int32), np.concatenate([g[70:71], g[:1]]), alpha)
    assert np.array_equal(n2, n) and np.array_equal(ok2, ok)
    assert not geo.ray_normals_host(w, bmw, Rs, idx, g, alpha, alpha_min=0.95)[1].any()


# ----------------------------------------------------------------------------------------------------------- panels
@pytest.mark.parametrize('H,W', [(1, 1), (5, 7), (16, 16)])
@pytest.mark.parametrize('surface', [0, 1])
def test_normal_panels_twin_against_fp64(H, W, surface):
    """Two rays on one pixel (the highest wins), pixels without a ray, rays without a normal, rays without a surface:
    the 8-bit panels are the truncation of the float64 value, up to one level where fp32 rounding crosses an integer."""
    c = nc.panel_case(H, W, seed=H * W + surface)
    p2r, st = geo.pixel_rays_host(c['ray_index'], H, W)
    assert st == 0
    got = geo.normal_panels_host(c['rays_d'], c['normal'], c['nvalid'], c['valid'], p2r, H, W, surface=surface,
                                 alpha=c['alpha'], M=c['M'], bgcolor=c['bgcolor'])
    n8, s8, has, ok = nc.panels_fp64(c, p2r, H, W, surface)
    assert sorted(got) == ['normal', 'normal8', 'nvalid', 'shaded8']
    assert np.array_equal(got['nvalid'].astype(bool), has)
    r = np.where(p2r.reshape(H, W) >= 0, p2r.reshape(H, W), 0)
    assert np.array_equal(got['normal'], np.where(has[..., None], c['normal'][r], np.float32(0)))
    for name, real in (('normal8', n8), ('shaded8', s8)):
        assert got[name].dtype == np.uint8 and got[name].shape == (H, W, 3)
        trunc = np.minimum(np.floor(real), 255)
        assert np.abs(got[name].astype(np.int64) - trunc).max() <= 1, name
        assert (got[name].astype(np.int64) != trunc).mean() <= 0.02, name
    bg8 = geo.q8_host(c['bgcolor'])
    assert (got['normal8'][~has] == bg8).all() and (got['shaded8'][~ok] == bg8).all()
    if H * W > 1:
        assert (~has).any() and has.any() and (p2r < 0).any()
        assert p2r[c['ray_index'][0]] == c['N'] - 1                           # the shared pixel shows the last ray
    only = geo.normal_panels_host(c['rays_d'], c['normal'], c['nvalid'], c['valid'], p2r, H, W, want=['shaded8'],
                                  surface=surface, alpha=c['alpha'], bgcolor=c['bgcolor'])
    assert list(only) == ['shaded8'] and np.array_equal(only['shaded8'], got['shaded8'])


def test_normal_panels_twin_paints_what_the_screen_space_twin_paints_for_the_same_normals():
    """Fed with the normals maps_host found itself, the panels are maps_host's, byte for byte: the q8 / M / ambient /
    albedo / alpha / background statements are the same ones."""
    import geometry_cases as gc
    H = W = 12
    rs = np.random.RandomState(5)
    o = np.zeros((H * W, 3), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.stack([(xx - W / 2) / 20, (yy - H / 2) / 20, np.ones((H, W))], -1).reshape(-1, 3).astype(np.float32)
    depth = (3 + 0.3 * np.sin(xx / 3.0) + 0.2 * np.cos(yy / 2.0)).reshape(-1).astype(np.float32)
    alpha = rs.uniform(0.4, 1.0, H * W).astype(np.float32)
    surf = geo.ray_surface_host(np.ones(H * W, np.float32), np.full(H * W, 5, np.float32), alpha, depth * alpha)
    p2r, _ = geo.pixel_rays_host(np.arange(H * W), H, W)
    M, bg = nc.rotations(1, rs)[0], np.array([0.1, 0.5, 0.9], np.float32)
    ref = geo.maps_host(o, d, surf, p2r, H, W, want=['normal', 'nvalid', 'normal8', 'shaded8'], alpha=alpha, M=M, bgcolor=bg)
    assert ref['nvalid'].any() and not ref['nvalid'].all()
    got = geo.normal_panels_host(d, ref['normal'].reshape(-1, 3), ref['nvalid'].reshape(-1), surf['valid'], p2r, H, W,
                                 alpha=alpha, M=M, bgcolor=bg)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
    assert gc is not None


# ---------------------------------------------------------------------------------------------------- field normals
def test_gate_gradient_twin_against_central_differences():
    """grad fg of the twin at 200 points away from the cell faces, inside the volume and in the zero-padded shell around
    it, against float64 central differences of an independently written trilinear gate: 2e-4 of the largest component
    (fp32 weights and 24 x 8 products against float64).  Far outside the volume both are exactly zero."""
    verts, _, _, vol, bmin, scale = nc.field_case(400, 24, 8, seed=2)
    keep = nc.away_from_faces(verts, bmin, scale, 8)
    verts = verts[keep][:200]
    assert len(verts) == 200
    i = (verts.astype(np.float64) - bmin) * scale * 0.5 * 7
    shell = ((i < 0) | (i > 7)).any(axis=1)
    assert shell.any() and (~shell).any()                                      # zero padding is exercised
    fg, grad = geo.trilinear_gradient_host(verts, vol, bmin, scale, 24)
    want_fg = np.array([nc.fg_fp64(x, vol, bmin, scale, 24) for x in verts.astype(np.float64)])
    h = 1e-6
    want = np.array([[(nc.fg_fp64(x + h * e, vol, bmin, scale, 24) - nc.fg_fp64(x - h * e, vol, bmin, scale, 24)) / (2 * h)
                      for e in np.eye(3)] for x in verts.astype(np.float64)])
    assert np.abs(fg - want_fg).max() <= 1e-5
    assert np.abs(grad - want).max() <= 2e-4 * np.abs(want).max()
    far = (bmin + np.array([[-5.0, 0.3, 0.2], [0.4, 9.0, 0.1]])).astype(np.float32)
    fg, grad = geo.trilinear_gradient_host(far, vol, bmin, scale, 24)
    assert (fg == 0).all() and (grad == 0).all()
    assert nc.fg_fp64(far[0].astype(np.float64), vol, bmin, scale, 24) == 0


def test_field_normals_twin_against_fp64():
    """77 vertices, densities of both signs: within 2e-4 per component of the float64 normal away from the cell faces;
    unit length or exactly zero; sigma <= 0 takes no gradient of sigma and, with relu(sigma) = 0, gives the zero normal."""
    verts, g, sigma, vol, bmin, scale = nc.field_case(77, 24, 8, seed=4)
    n = geo.field_normals_host(verts, g, sigma, vol, bmin, scale, 24)
    want = nc.field_normals_fp64(verts, g, sigma, vol, bmin, scale, 24)
    keep = nc.away_from_faces(verts, bmin, scale, 8)
    assert n.dtype == np.float32 and n.shape == (77, 3) and keep.sum() > 60
    assert np.abs(n[keep] - want[keep]).max() <= 2e-4
    lens = np.linalg.norm(n.astype(np.float64), axis=1)
    assert ((lens == 0) | (np.abs(lens - 1) <= 2.0 ** -22)).all()
    assert (n[sigma <= 0] == 0).all() and (lens[sigma > 0] > 0).sum() > 20
    assert geo.field_normals_host(verts[:0], g[:0], sigma[:0], vol, bmin, scale, 24).shape == (0, 3)


# ------------------------------------------------------------------------------------------ the gradient's definition
@pytest.mark.parametrize('seed', [11, 12, 13])
def test_density_gradient_reference_is_autograd_of_the_oracle_sigma(seed):
    """The fp64 reference the GPU test uses -- ref_mlp_grads with g = (0, 0, 0, 1) -- is torch.autograd of
    oracle.canonical_mlp's sigma, and on these weights no sample has a gradient below 1 % of the largest: the exclusion
    rule of the GPU test leaves nothing out."""
    from oracle import oracle
    from tests.test_train_kernel_refs import make_problem, ref_mlp, ref_mlp_grads
    P = 1000
    pr = make_problem('canonical', P, seed)
    g = np.zeros((P, 4), np.float32)
    g[:, 3] = 1
    fwd = ref_mlp(pr)
    masks = [(a > 0).double() for a in fwd['acts']]
    ref = ref_mlp_grads(pr, masks, g)['d_x'].numpy()
    x = torch.from_numpy(pr['x']).double().requires_grad_(True)
    sigma = oracle.canonical_mlp({k: torch.from_numpy(v).double() for k, v in pr['st'].items()}, oracle.fourier_pe(x, 10))[:, 3]
    sigma.sum().backward()
    auto = x.grad.numpy()
    assert np.abs(ref - auto).max() <= 1e-9 * np.abs(auto).max()
    norm = np.linalg.norm(ref, axis=1)
    print('|grad sigma| median %.1f max %.1f min %.2f' % (np.median(norm), norm.max(), norm.min()))
    assert (norm < 0.01 * norm.max()).mean() == 0.0


# ------------------------------------------------------------------------------------------------------- the options
def test_check_amd_options_for_normals():
    from humannerf_amd.config import _DEFAULTS, check_amd_options
    assert _DEFAULTS['amd']['maps_normals'] == 'screen' and _DEFAULTS['amd']['normal_weight_min'] == 1e-4
    check_amd_options({})
    check_amd_options({'maps_normals': 'gradient', 'maps': ['normal', 'shaded'], 'normal_weight_min': 1e-3})
    check_amd_options({'maps_normals': 'screen', 'diagnostics': False})
    with pytest.raises(ValueError, match='maps_normals'):
        check_amd_options({'maps_normals': 'sobel'})
    for bad in (0, 0.0, -1e-4, float('inf'), float('nan'), '1e-4', None, True):
        with pytest.raises(ValueError, match='normal_weight_min'):
            check_amd_options({'normal_weight_min': bad})
    with pytest.raises(ValueError) as e:
        check_amd_options({'maps_normals': 'gradient', 'diagnostics': False})
    assert 'cfg.amd.maps_normals' in str(e.value) and 'cfg.amd.diagnostics = True' in str(e.value)
    assert geo.MAP_NAMES == ('depth', 'normal', 'shaded', 'offset')
    assert geo.OUTPUTS == ('normal', 'nvalid', 'normal8', 'depth8', 'shaded8', 'offset8')


# --------------------------------------------------------------------------------------------------------- the files
def _mesh(V=7):
    rs = np.random.RandomState(1)
    verts = rs.standard_normal((V, 3)).astype(np.float32)
    faces = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6]], np.int32)
    colors = rs.uniform(0, 1, (V, 3)).astype(np.float32)
    n = rs.standard_normal((V, 3))
    normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    normals[3] = 0                                                             # (where the field has no gradient)
    return verts, faces, colors, normals


@pytest.mark.parametrize('with_colors', [True, False])
def test_ply_round_trips_normals(tmp_path, with_colors):
    from humannerf_amd import mesh
    verts, faces, colors, normals = _mesh()
    col = colors if with_colors else None
    a, b, c = str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply'), str(tmp_path / 'c.ply')
    mesh.write_ply(a, verts, faces, col)
    mesh.write_ply(b, verts, faces, col, normals=None)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    mesh.write_ply(c, verts, faces, col, normals=torch.from_numpy(normals))
    v, f, k, n = mesh.read_ply(c, want_normals=True)
    assert np.array_equal(v, verts) and np.array_equal(f, faces) and np.array_equal(n, normals) and (k is None) == (col is None)
    head = open(c, 'rb').read().split(b'end_header')[0].decode()
    assert head.index('property float z') < head.index('property float nx') < head.index('property float nz')
    if with_colors:
        assert head.index('property float nz') < head.index('property uchar red')
        assert np.array_equal(k, mesh.read_ply(a)[2])
    assert len(mesh.read_ply(c)) == 3 and np.array_equal(mesh.read_ply(c)[0], verts)
    assert mesh.read_ply(a, want_normals=True)[3] is None
    with pytest.raises(ValueError, match='normals'):
        mesh.write_ply(c, verts, faces, col, normals=normals[:3])


def test_glb_round_trips_normals(tmp_path):
    from humannerf_amd import gltf
    from humannerf_amd.scene import SMPL_PARENT
    verts, faces, colors, normals = _mesh()
    J = len(SMPL_PARENT)
    rs = np.random.RandomState(2)
    joints = rs.randint(0, J, (7, 4)).astype(np.uint8)
    weights = rs.uniform(0, 1, (7, 4)).astype(np.float32)
    weights /= weights.sum(1, keepdims=True)
    g = np.tile(np.eye(4), (J, 1, 1))
    g[:, :3, 3] = rs.standard_normal((J, 3)) * 0.3
    R = np.tile(np.eye(3), (2, J, 1, 1))
    Ts = np.tile(g[None, :, :3, 3], (2, 1, 1)).astype(np.float32)
    kw = dict(dst_Rs=R, dst_Ts=Ts, Rh=np.zeros((2, 3)), Th=np.zeros((2, 3)))
    a, b, c = str(tmp_path / 'a.glb'), str(tmp_path / 'b.glb'), str(tmp_path / 'c.glb')
    gltf.write_glb(a, verts, faces, colors, joints, weights, g, **kw)
    gltf.write_glb(b, verts, faces, colors, joints, weights, g, normals=None, **kw)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    gltf.write_glb(c, verts, faces, colors, joints, weights, g, normals=normals, **kw)
    plain, glb = gltf.read_glb(a), gltf.read_glb(c)
    assert 'normals' not in plain and 'NORMAL' not in plain['json']['meshes'][0]['primitives'][0]['attributes']
    acc = glb['json']['accessors'][glb['json']['meshes'][0]['primitives'][0]['attributes']['NORMAL']]
    assert acc['type'] == 'VEC3' and acc['componentType'] == gltf.FLOAT and acc['count'] == 7
    assert np.array_equal(glb['normals'], normals)
    assert np.allclose(gltf.pose(glb, 1), gltf.pose(plain, 1)) and np.array_equal(gltf.pose(glb), gltf.pose(plain))
    for bad in (normals[:3], np.full((7, 3), np.nan, np.float32)):
        with pytest.raises(ValueError, match='normals'):
            gltf.write_glb(c, verts, faces, colors, joints, weights, g, normals=bad, **kw)


# ------------------------------------------------------------------------------------------------------- the binding
def test_normals_group_is_bound_like_the_other_additive_headers():
    from humannerf_amd import _lib
    assert 'normals' in _lib.OPEN_GROUPS and _lib.OPEN_GROUPS['normals'][0] == 'hnrf_normals.h'
    names = {'hnrf_ray_normals_workspace_bytes', 'hnrf_ray_normals', 'hnrf_normal_panels', 'hnrf_field_normals'}
    assert set(_lib.NORMALS_SIGNATURES) == names
    assert not names & set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 88
    assert len(_lib.NORMALS_SIGNATURES['hnrf_ray_normals'][1]) == 17

    class Old:                                                                 # a library built before the header
        pass
    with pytest.raises(_lib.HnrfError, match='hnrf_normals.h.*rebuild'):
        _lib.load_normals(Old())
    header = open(_lib.HEADER_PATH).read()
    assert '#include "hnrf_normals.h"' in header
