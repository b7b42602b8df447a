"""Geometry maps on the MI355X (include/hnrf_geometry.h, csrc/hnrf_geometry.hip): every kernel against its numpy twin
(humannerf_amd/geometry.py) BIT FOR BIT on every output, the panels of render_frames(maps=...) against the twin run on the
frame's own outputs, and the two loops of run.py.  The twins themselves are held against independent statements in
tests/test_geometry_refs.py."""
import glob
import os

import numpy as np
import pytest
import torch

import geometry_cases as gc
from humannerf_amd import geometry as geo

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def T(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def same(a, b):
    """Bit for bit; a NaN equals a NaN (the twin's and the device's NaNs may differ in sign and payload)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def dev_surface(near, far, alpha, depth, w=None, off=None, median=False, woff=False, alpha_min=0.5):
    from humannerf_amd import ops
    res = ops.ray_surface(T(near), T(far), T(alpha), T(depth), T(w), T(off), alpha_min=alpha_min, want_median=median,
                          want_woff=woff)
    return {k: v.cpu().numpy() for k, v in res.items()}


# --------------------------------------------------------------------------------------------------- hnrf_ray_surface
@pytest.mark.parametrize('S', gc.S_LIST)
@pytest.mark.parametrize('R', [1, 3, 4, 5, 1000])
def test_ray_surface_equals_twin(R, S):
    """R around the four rays of a workgroup and a ragged last one; S around the 64-sample tile; the special rows of
    geometry_cases.surface_inputs (zero, one-hot, NaN weights, near == far, alpha at alpha_min, non-finite alpha / depth);
    the full form, the forms that ask for one product only, and the lean form."""
    near, far, alpha, depth, w, off = gc.surface_inputs(R, S, seed=100 * R + S)
    want = geo.ray_surface_host(near, far, alpha, depth, w, off, want_median=True, want_woff=True)
    got = dev_surface(near, far, alpha, depth, w, off, median=True, woff=True)
    for k in ('t_exp', 't_med', 'woff', 'valid'):
        assert same(got[k], want[k]), k
    only_m = dev_surface(near, far, alpha, depth, w, None, median=True)
    assert sorted(only_m) == ['t_exp', 't_med', 'valid'] and same(only_m['t_med'], want['t_med']) and same(only_m['valid'], want['valid'])
    only_w = dev_surface(near, far, alpha, depth, w, off, woff=True)
    assert same(only_w['woff'], want['woff']) and same(only_w['valid'], want['valid'] & 1) and same(only_w['t_exp'], want['t_exp'])
    lean = dev_surface(near, far, alpha, depth)
    assert sorted(lean) == ['t_exp', 'valid'] and same(lean['t_exp'], want['t_exp']) and same(lean['valid'], want['valid'] & 1)
    other = geo.ray_surface_host(near, far, alpha, depth, alpha_min=0.25)
    assert same(dev_surface(near, far, alpha, depth, alpha_min=0.25)['valid'], other['valid'])


def test_ray_surface_refusals():
    from humannerf_amd import ops
    from humannerf_amd._lib import HnrfError
    near, far, alpha, depth, w, off = (T(v) for v in gc.surface_inputs(8, 16, seed=1))
    with pytest.raises(HnrfError, match='t_med needs weights'):
        ops.ray_surface(near, far, alpha, depth, None, None, want_median=True)
    with pytest.raises(HnrfError, match='woff needs weights and offsets'):
        ops.ray_surface(near, far, alpha, depth, w, None, want_woff=True)
    with pytest.raises(HnrfError, match='alpha_min'):
        ops.ray_surface(near, far, alpha, depth, alpha_min=float('nan'))
    with pytest.raises(HnrfError):
        ops.ray_surface(near, far, alpha.double(), depth)
    empty = ops.ray_surface(near[:0], far[:0], alpha[:0], depth[:0], w[:0], off[:0], want_median=True, want_woff=True)
    assert empty['t_med'].numel() == 0


# ---------------------------------------------------------------------------------------------------- hnrf_pixel_rays
def _pixel_rays(idx, H, W, fill):
    from humannerf_amd import ops
    pix = torch.full((H * W,), fill, dtype=torch.int32, device=DEV)
    st = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    ops.pixel_rays(T(np.asarray(idx, np.int64)), H, W, pix2ray=pix, status=st)
    return pix.cpu().numpy(), int(st.item())


@pytest.mark.parametrize('H,W', [(1, 1), (1, 7), (2, 2), (17, 33)])
def test_pixel_rays_equals_twin(H, W):
    rs = np.random.RandomState(H * 100 + W)
    HW = H * W
    cases = [np.zeros(0, np.int64), np.arange(HW), rs.permutation(HW)[:max(1, HW // 2)], rs.permutation(HW)]
    cases.append(np.concatenate([cases[2], cases[2][:1], cases[2][:1]]))         # a pixel with three rays
    cases.append(rs.randint(0, HW, 3 * HW))                                        # many duplicates: the highest ray wins
    for idx in cases:
        want, st = geo.pixel_rays_host(idx, H, W)
        assert st == 0
        a, sa = _pixel_rays(idx, H, W, -1)                                         # a workspace of 0xFF bytes ...
        b, sb = _pixel_rays(idx, H, W, 0)                                          # ... and one of zeros
        assert sa == 0 and sb == 0 and same(a, want) and same(b, want)
    for bad in ([HW], [-1], list(range(HW)) + [HW + 5]):
        assert geo.pixel_rays_host(bad, H, W) == (None, 1)
        a, sa = _pixel_rays(bad, H, W, 12345)
        assert sa == 1 and (a == 12345).all()                                      # status set, nothing else written


def test_maps_write_nothing_under_a_raised_status():
    from humannerf_amd import ops
    H, W = 5, 6
    o, d, surf, p2r = gc.full_frame(H, W, np.full(H * W, 3.0))
    out = {k: torch.full((H, W, 3), 9, dtype=torch.uint8, device=DEV) for k in ('depth8', 'normal8')}
    st = torch.ones(1, dtype=torch.int32, device=DEV)
    ops.geometry_maps(T(o), T(d), {k: T(v) for k, v in surf.items()}, T(p2r), H, W, ['depth8', 'normal8'], M=T(np.eye(3, dtype=np.float32)),
                      bgcolor=T(np.zeros(3, np.float32)), lohi=T(np.array([2, 4], np.float32)), status=st, out=out)
    assert all(bool((v == 9).all()) for v in out.values())


# ------------------------------------------------------------------------------------------------- hnrf_geometry_maps
def _rotation(seed):
    q, _ = np.linalg.qr(np.random.RandomState(seed).normal(size=(3, 3)))
    return q.astype(np.float32)


def _dev_maps(o, d, surf, p2r, H, W, want, **kw):
    from humannerf_amd import ops
    conv = {k: (T(np.asarray(v, np.float32)) if k in ('alpha', 'M', 'bgcolor', 'lohi') else T(v) if k == 'truth8' else v)
            for k, v in kw.items()}
    res = ops.geometry_maps(T(o), T(d), {k: T(v) for k, v in surf.items()}, T(np.asarray(p2r, np.int32)), H, W, list(want), **conv)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _check_all(o, d, surf, p2r, H, W, each_alone=False, **kw):
    want = geo.maps_host(o, d, surf, p2r, H, W, want=geo.OUTPUTS, **kw)
    got = _dev_maps(o, d, surf, p2r, H, W, geo.OUTPUTS, **kw)
    for k in geo.OUTPUTS:
        assert same(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    if each_alone:
        for k in geo.OUTPUTS:
            alone = _dev_maps(o, d, surf, p2r, H, W, [k], **kw)
            assert list(alone) == [k] and same(alone[k], want[k]), k
    return want


def _scene_kw(H, W, seed=0):
    rs = np.random.RandomState(seed)
    return dict(alpha=rs.uniform(0.5, 1.0, H * W).astype(np.float32), M=_rotation(seed), bgcolor=(0.2, 0.5, 1.0),
                lohi=(2.4, 3.4))


@pytest.mark.parametrize('scene', ['plane0', 'plane1', 'plane2', 'plane3', 'sphere', 'step', 'step_wide', 'island'])
def test_maps_equal_twin_on_the_analytic_scenes(scene):
    """The scenes of tests/test_geometry_refs.py: the device gives the twin's bits, so what that file shows of the twin
    (the normals' accuracy, the one-sided rule, the island) holds for the kernel."""
    edge, hit = 0.05, None
    if scene.startswith('plane'):
        H, W, edge = 17, 33, 1e9
        t64 = gc.plane_t(gc.PLANES[int(scene[-1])], 0.0, H, W)
    elif scene == 'sphere':
        H = W = 32
        t64, hit = gc.sphere_t(0.5, H, W)
    elif scene.startswith('step'):
        H, W = 9, 16
        t64, edge = gc.step_t(H, W, 8), (1.0 if scene == 'step_wide' else 0.05)
    else:
        H, W = 5, 7
        t64, hit = np.full(H * W, 3.0), np.zeros((H, W), bool)
        hit[2, 3] = True
    o, d, surf, p2r = gc.full_frame(H, W, t64, hit)
    surf['woff'] = np.random.RandomState(5).normal(0, 0.015, (H * W, 3)).astype(np.float32)
    res = _check_all(o, d, surf, p2r, H, W, edge=edge, **_scene_kw(H, W))
    assert res['nvalid'].any() == (scene != 'island')


def _random_field(H, W, seed):
    """A frame whose rays are a shuffled subset of the pixels: 10 % of the pixels have no ray, 30 % of the rays are
    invalid for either surface, t is a slope with jumps (so that neighbours fall on both sides of ``edge``), with NaN
    and +-inf at a few VALID rays."""
    rs = np.random.RandomState(seed)
    pix = np.sort(rs.permutation(H * W)[:max(1, int(0.9 * H * W))])
    N = pix.size
    o = np.tile(gc.CAM, (N, 1)).astype(np.float32) + rs.normal(0, 1e-3, (N, 3)).astype(np.float32)
    d = gc.camera(H, W)[1][pix].astype(np.float32)
    y, x = pix // W, pix % W
    t = (3.0 + 0.004 * x - 0.003 * y + 0.08 * (rs.uniform(size=N) < 0.15) * rs.normal(size=N)).astype(np.float32)
    t2 = (t + rs.normal(0, 0.01, N)).astype(np.float32)
    valid = ((rs.uniform(size=N) > 0.3) * 1 + (rs.uniform(size=N) > 0.3) * 2).astype(np.uint8)
    for k, v in enumerate((np.nan, np.inf, -np.inf) if N > 30 else ()):
        t[5 + 7 * k], t2[9 + 7 * k] = v, v
        valid[5 + 7 * k] = valid[9 + 7 * k] = 3
    surf = {'t_exp': t, 't_med': t2, 'valid': valid, 'woff': rs.normal(0, 0.015, (N, 3)).astype(np.float32)}
    surf['woff'][N // 2] = (np.nan, 1.0, -1.0)
    p2r, st = geo.pixel_rays_host(pix, H, W)
    assert st == 0
    truth = (rs.randint(0, 256, (H, W, 3)) * (rs.uniform(size=(H, W, 1)) > 0.4)).astype(np.uint8)
    kw = dict(alpha=rs.uniform(0.0, 1.0, N).astype(np.float32), M=_rotation(seed), bgcolor=(0.2, 0.5, 1.0), edge=0.05)
    return o, d, surf, p2r, truth, kw


@pytest.mark.parametrize('H,W', [(17, 33), (64, 64), (1, 1), (1, 70), (67, 1), (5, 130)])
def test_maps_equal_twin_on_random_fields(H, W):
    """More than one workgroup in both directions, sizes that are no multiple of the 64 x 4 tile, single rows and
    columns (the first and last row and column are every pixel's neighbours there); both surfaces; lo == hi; with and
    without a truth; every panel alone at the first size."""
    o, d, surf, p2r, truth, kw = _random_field(H, W, seed=H * 1000 + W)
    res = _check_all(o, d, surf, p2r, H, W, each_alone=(H, W) == (17, 33), surface=0, lohi=(2.9, 3.4), truth8=truth, **kw)
    if min(H, W) >= 17:
        assert res['nvalid'].any() and not res['nvalid'].all()
        for edge_px in (res['nvalid'][0], res['nvalid'][-1], res['nvalid'][:, 0], res['nvalid'][:, -1]):
            assert edge_px.any()                                 # the border has normals: one-sided differences
    _check_all(o, d, surf, p2r, H, W, surface=1, lohi=(3.0, 3.0), truth8=None, **kw)
    _check_all(o, d, surf, p2r, H, W, surface=1, lohi=(2.9, 3.4), truth8=truth, **dict(kw, edge=0.0))


# ------------------------------------------------------------------------------------------------------- the loops
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
    root = str(tmp_path_factory.mktemp('geometry') / 'subject')
    names = scene.write_synthetic_subject(root, n_frames=3, size=32)
    return dataset.Subject(root), names


@pytest.fixture()
def loop_cfg():
    from humannerf_amd.config import cfg
    amd = cfg.amd
    keys = ('metrics', 'video', 'maps', 'maps_surface', 'canonical', 'bake_resolution', 'diagnostics')
    old = (cfg.get('show_truth', False), cfg.get('show_alpha', False), cfg.N_samples, cfg.ignore_non_rigid_motions,
           {k: amd[k] for k in keys if k in amd})
    cfg.N_samples, cfg.show_alpha, amd.diagnostics = 16, True, True
    yield cfg
    cfg.show_truth, cfg.show_alpha, cfg.N_samples, cfg.ignore_non_rigid_motions = old[:4]
    for k in keys:
        if k in old[4]:
            amd[k] = old[4][k]
        else:
            amd.pop(k, None)


def _frames(subject):
    from humannerf_amd import run
    return run._Frames(len(subject), lambda i: subject.movement_frame(i, load_image=True, device=DEV))


def _render(net, subject, monkeypatch, maps, video=None):
    """render_frames over the subject's frames -> (images {idx: arrays}, panels {idx: {name: array}}, the recorded
    inputs of every geometry.frame_maps call, streams {idx: bytes})."""
    from humannerf_amd import render
    calls, images, panels, streams = [], {}, {}, {}
    real = geo.frame_maps

    def spy(data, out, H, W, ray_index, **kw):
        host = lambda v: v.detach().cpu().numpy().copy() if torch.is_tensor(v) else v
        calls.append(dict(data={k: host(v) for k, v in data.items() if k in ('rays', 'near', 'far', 'bgcolor')},
                          out={k: host(v) for k, v in out.items() if k in ('alpha', 'depth', 'weights_on_rays', 'offsets')},
                          H=H, W=W, ray_index=host(ray_index), kw={k: host(v) for k, v in kw.items()}))
        return real(data, out, H, W, ray_index, **kw)

    monkeypatch.setattr(geo, 'frame_maps', spy)
    extra = {}
    if maps:
        extra.update(maps=maps, on_maps=lambda i, p: panels.__setitem__(i, p))
    if video is not None:
        extra.update(video=video, on_video=lambda i, b: streams.__setitem__(i, b))
    render.render_frames(net, _frames(subject), device=DEV, show_truth=True,
                         on_image=lambda i, *a: images.__setitem__(i, [x.copy() for x in a]), **extra)
    return images, panels, calls, streams


def _twin_panels(call, maps):
    """geometry.maps_host on what one frame_maps call was given."""
    d, o, kw = call['data'], call['out'], call['kw']
    median = kw['surface'] == 'median'
    N = o['alpha'].reshape(-1).shape[0]
    w = o['weights_on_rays'].reshape(N, -1) if 'weights_on_rays' in o else None
    surf = geo.ray_surface_host(d['near'], d['far'], o['alpha'], o['depth'], w if (median or 'offset' in maps) else None,
                                o.get('offsets') if 'offset' in maps else None, want_median=median,
                                want_woff='offset' in maps)
    p2r, st = geo.pixel_rays_host(call['ray_index'], call['H'], call['W'])
    assert st == 0
    lohi = (d['near'].min(), d['far'].max())
    names = {'depth': 'depth8', 'normal': 'normal8', 'shaded': 'shaded8', 'offset': 'offset8'}
    res = geo.maps_host(d['rays'][0], d['rays'][1], surf, p2r, call['H'], call['W'], want=[names[m] for m in maps],
                        surface=int(median), alpha=o['alpha'], edge=0.05, M=kw['M'] if kw.get('M') is not None else np.eye(3),
                        bgcolor=(d['bgcolor'].astype(np.float32) / np.float32(255.)), lohi=lohi, truth8=kw.get('truth8'))
    return {m: res[names[m]] for m in maps}, surf


@pytest.mark.parametrize('path', ['exact', 'baked'])
def test_render_frames_maps(path, net, subject, loop_cfg, monkeypatch):
    """Seeded network, 32 x 32 frames, S = 16: the panels equal the twin run on the frame's own outputs, on_image gets
    the bytes it gets without maps, and the video shows the maps behind the other panels."""
    from humannerf_amd import run, video as hvideo
    sub, names = subject
    maps = ['depth', 'normal', 'shaded', 'offset']
    loop_cfg.show_truth = True                       # (what run_movement sets: the truth panel is shown)
    if path == 'baked':
        loop_cfg.amd.canonical, loop_cfg.amd.bake_resolution = 'baked', 32
        run._baked_folder(net, sub, 'movement')
    plain, none, calls0, _ = _render(net, sub, monkeypatch, None)
    assert none == {} and calls0 == []
    enc = hvideo.JpegEncoder(DEV, 90)
    images, panels, calls, streams = _render(net, sub, monkeypatch, maps, video=enc)
    assert sorted(images) == sorted(plain) == [0, 1, 2] and sorted(panels) == [0, 1, 2] and len(calls) == 3
    for i in plain:
        assert len(images[i]) == len(plain[i]) == 3
        assert all(a.tobytes() == b.tobytes() for a, b in zip(images[i], plain[i]))
    for call, i in zip(calls, sorted(panels)):
        want, surf = _twin_panels(call, maps)
        assert list(panels[i]) == maps
        for m in maps:
            assert panels[i][m].shape == (32, 32, 3) and same(panels[i][m], want[m]), (i, m)
        assert (surf['valid'] & 1).any()                                     # the frames show a surface
        h, w = hvideo.jpeg_size(streams[i])
        assert (w, h) == (32 * (3 + len(maps)), 32)                          # [render | truth | alpha | maps...]
    for surface in ('median',):
        loop_cfg.amd.maps_surface = surface
        _, panels2, calls2, _ = _render(net, sub, monkeypatch, ['depth', 'normal'])
        for call, i in zip(calls2, sorted(panels2)):
            want, surf = _twin_panels(call, ['depth', 'normal'])
            assert all(same(panels2[i][m], want[m]) for m in want) and (surf['valid'] & 2).any()
    loop_cfg.amd.maps_surface = 'expected'
    loop_cfg.amd.diagnostics = False                                         # the lean form: t_exp only
    _, panels3, calls3, _ = _render(net, sub, monkeypatch, ['depth', 'normal', 'shaded'])
    for call, i in zip(calls3, sorted(panels3)):
        assert 'weights_on_rays' not in call['out']
        want, _ = _twin_panels(call, ['depth', 'normal', 'shaded'])
        assert all(same(panels3[i][m], want[m]) for m in want)
    from humannerf_amd import render
    with pytest.raises(ValueError, match='diagnostics'):
        render.render_frames(net, _frames(sub), device=DEV, maps=['offset'])
    with pytest.raises(ValueError, match='GPU'):
        render.render_frames(net, _frames(sub), device=torch.device('cpu'), maps=['depth'])


def _tree(root):
    out = {}
    for p in sorted(glob.glob(os.path.join(root, '**', '*'), recursive=True)):
        if os.path.isfile(p):
            with open(p, 'rb') as f:
                out[os.path.relpath(p, root)] = f.read()
    return out


def test_run_movement_without_maps_writes_the_same_bytes(net, subject, loop_cfg, tmp_path):
    """cfg.amd.maps = [] against the key absent: every file the same; with maps the PNG grows by the panels."""
    from PIL import Image
    from humannerf_amd import run
    sub, names = subject
    loop_cfg.amd.pop('maps', None)
    run.run_movement(net, sub, logdir=str(tmp_path / 'absent'), metrics=['psnr'])
    loop_cfg.amd.maps = []
    run.run_movement(net, sub, logdir=str(tmp_path / 'empty'), metrics=['psnr'])
    a, b = _tree(str(tmp_path / 'absent')), _tree(str(tmp_path / 'empty'))
    assert a == b and sum(k.endswith('.png') for k in a) == 3
    loop_cfg.amd.maps = ['depth', 'normal']
    res = run.run_movement(net, sub, logdir=str(tmp_path / 'maps'), metrics=['psnr'])
    c = _tree(str(tmp_path / 'maps'))
    assert sorted(c) == sorted(a)
    for k in a:
        if k.endswith('.png'):
            small, big = np.asarray(Image.open(os.path.join(str(tmp_path / 'absent'), k))), np.asarray(Image.open(os.path.join(str(tmp_path / 'maps'), k)))
            assert small.shape == (32, 96, 3) and big.shape == (32, 160, 3) and np.array_equal(big[:, :96], small)
        elif k.endswith('.txt'):
            assert c[k] == a[k]
    assert sorted(res['images']) == [0, 1, 2]


def test_run_compare_lbs_delta(net, subject, loop_cfg, tmp_path, monkeypatch):
    """Three files [lbs | full | offset | truth] whose names carry the PSNRs MetricsWriter reports for the two renders;
    the third panel is the twin's offset8 of the full render; the flags it touches are restored."""
    from PIL import Image
    from humannerf_amd import run
    from humannerf_amd.config import cfg
    sub, names = subject
    calls = []
    real = geo.frame_maps

    def spy(data, out, H, W, ray_index, **kw):
        host = lambda v: v.detach().cpu().numpy().copy() if torch.is_tensor(v) else v
        calls.append(dict(data={k: host(v) for k, v in data.items() if k in ('rays', 'near', 'far', 'bgcolor')},
                          out={k: host(v) for k, v in out.items() if k in ('alpha', 'depth', 'weights_on_rays', 'offsets')},
                          H=H, W=W, ray_index=host(ray_index), kw={k: host(v) for k, v in kw.items()}))
        return real(data, out, H, W, ray_index, **kw)

    monkeypatch.setattr(geo, 'frame_maps', spy)
    loop_cfg.amd.diagnostics = False
    cfg.ignore_non_rigid_motions = False
    res = run.run_compare_lbs_delta(net, sub, logdir=str(tmp_path))
    assert cfg.amd.diagnostics is False and cfg.ignore_non_rigid_motions is False
    files = sorted(os.listdir(res['image_dir']))
    assert len(files) == 3 and len(res['lbs']) == len(res['full']) == 3 and len(calls) == 3
    base = os.path.join(str(tmp_path), os.path.relpath(os.path.dirname(res['image_dir']), str(tmp_path)))
    scores = {}
    for tag in ('lbs', 'full'):
        with open(os.path.join(base, 'movement_%s-metrics.perimg.txt' % tag)) as f:
            lines = [l.strip() for l in f if ': psnr-' in l]
        scores[tag] = {l.split(':')[0]: float(l.split('psnr-')[1].split()[0]) for l in lines}
    for i, name in enumerate(sorted(n.replace('/', '-') for n in names)):
        j = res['names'].index(name)
        assert abs(scores['lbs'][name] - res['lbs'][j]) < 1e-4 and abs(scores['full'][name] - res['full'][j]) < 1e-4
        fn = '%s_lbs-%.1f_full-%.1f.png' % (name, res['lbs'][j], res['full'][j])
        assert fn in files
        img = np.asarray(Image.open(os.path.join(res['image_dir'], fn)))
        assert img.shape == (32, 128, 3)
        want, _ = _twin_panels(calls[j], ['offset'])
        assert same(img[:, 64:96], want['offset']) and img[:, 64:96].any()
    assert res['lbs'] != res['full']                                         # the non-rigid motions change the picture
