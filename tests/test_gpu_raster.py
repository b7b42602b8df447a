"""The rasteriser on the MI355X: hnrf_raster_mesh against its numpy restatement bit for bit (both instances of the
visibility kernel, the bbox clamp, every cull and shade), run-to-run determinism under the atomics, screen-filling
triangles, Network.render_mesh and run.run_mesh_render on a synthetic subject."""
import os
import time

import numpy as np
import pytest
import torch

import test_raster_cpu as cases
from humannerf_amd import mesh, raster, scene
from humannerf_amd._lib import HnrfError
from humannerf_amd.config import cfg
from humannerf_amd.network import Network
from humannerf_amd.seeded import default_shapes, seeded_state, with_density

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
LEVEL = 10.0                                # as tests/test_gpu_mesh.py: the seeded state with the sigma bias raised by 5
OUTPUTS = ('rgb', 'alpha', 'depth', 'tri_id')
SETTINGS = [(cull, shade) for cull in ('none', 'back', 'front') for shade in ('color', 'normal')]


def on_device(verts, faces, colors, K, E, H, W, **kw):
    d = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=t)
    return raster.rasterize(d(verts, torch.float32), d(faces, torch.int32), d(colors, torch.float32), K, E, H, W, **kw)


def assert_same(dev, host, what):
    for k in OUTPUTS:
        got = dev[k].cpu()
        assert got.dtype == torch.from_numpy(host[k]).dtype and got.shape == host[k].shape, (what, k)
        # (bit patterns: NaN-proof and -0.0-proof)
        assert torch.equal(got.view(torch.int32), torch.from_numpy(host[k]).view(torch.int32)), (what, k)


def build_case(name):
    """-> list of (label, verts, faces, colors, K, E, H, W)"""
    if name in ('sphere128', 'sphere256'):
        size = int(name[6:])
        v, f = cases.sphere_mesh()
        return [(name, v, f, cases.vertex_colors(v), *cases.tpose_camera(size), size, size)]
    if name == 'torus':
        v, f = cases.field_mesh(64, lambda x, y, z: 0.04 - (np.sqrt(x * x + y * y) - 0.5) ** 2 - z * z)
        return [(name, v, f, cases.vertex_colors(v), *cases.tpose_camera(128), 128, 128)]
    if name == 'two_spheres':
        v, f = cases.field_mesh(64, lambda x, y, z: np.maximum(0.3 - np.sqrt((x - 0.45) ** 2 + y * y + z * z),
                                                               0.3 - np.sqrt((x + 0.45) ** 2 + y * y + z * z)))
        return [(name, v, f, cases.vertex_colors(v), *cases.tpose_camera(128), 128, 128)]
    if name == 'wide':                      # not square, and the body cut by the right and bottom borders
        v, f = cases.field_mesh(64, lambda x, y, z: 0.04 - (np.sqrt(x * x + y * y) - 0.5) ** 2 - z * z)
        return [(name, v, f, cases.vertex_colors(v), *cases.tpose_camera(160), 96, 136),
                (name + ' tall', v, f, cases.vertex_colors(v), *cases.tpose_camera(160), 150, 72)]
    if name == 'mirrored':                  # det(K R) < 0: the facing flips on the device too
        v, f = cases.field_mesh(32, lambda x, y, z: 0.6 - np.sqrt(x * x + y * y + z * z))
        K, E = cases.tpose_camera(64)
        K = K.copy()
        K[0, 0], K[0, 2] = -K[0, 0], 63.0 - K[0, 2]
        assert raster.camera_flips(K, E[:3, :3])
        return [(name, v, f, cases.vertex_colors(v), K, E, 64, 64)]
    if name == 'polygons':
        out = []
        for n, (c, p) in enumerate(cases.polygons(120)):
            v, fans = cases.polygon_meshes(c, p)
            for fan, f in fans.items():
                out.append(('polygon %d %s' % (n, fan), v, f, cases.vertex_colors(v), cases.EYE_K, cases.EYE_E, 64, 64))
        return out
    assert name == 'soup'
    v, f = cases.soup()
    return [(name, v, f, cases.vertex_colors(v), cases.EYE_K, cases.EYE_E, 256, 256)]


CASES = ['sphere128', 'sphere256', 'torus', 'two_spheres', 'wide', 'mirrored', 'polygons', 'soup']


@pytest.mark.parametrize('name', CASES)
def test_device_equals_host_bit_for_bit(name):
    for label, v, f, col, K, E, H, W in build_case(name):
        covered = 0
        for cull, shade in SETTINGS:
            kw = dict(bgcolor=(0.25, 0.5, 0.75), cull=cull, shade=shade)
            host = raster.rasterize_host(v, f, col, K, E, H, W, **kw)
            assert_same(on_device(v, f, col, K, E, H, W, **kw), host, (label, cull, shade))
            covered += int((host['tri_id'] >= 0).sum())
        assert covered > 0, label
    if name == 'soup':                      # both instances of the visibility kernel and the clamp were exercised
        X, Y, w, ok = raster.project_host(v, K, E)
        okf = ok[f].all(1)
        ext = lambda A: (A[f].max(1) >> 8) - ((A[f].min(1) + 255) >> 8) + 1
        n = np.where(okf, np.maximum(ext(X), 0) * np.maximum(ext(Y), 0), 0)
        assert (n > 64).sum() > 1000 and ((n > 0) & (n <= 64)).sum() > 1000 and (~okf).sum() > 100
        off = okf & ((X[f].min(1) < 0) | (X[f].max(1) > 255 * 256) | (Y[f].min(1) < 0) | (Y[f].max(1) > 255 * 256))
        assert off.sum() > 1000


@pytest.mark.parametrize('name', CASES)
def test_outputs_do_not_change_from_run_to_run(name):
    other = build_case('torus')[0]
    built = build_case(name)
    for label, v, f, col, K, E, H, W in built[::7]:                    # (every seventh polygon fan; the others whole)
        for cull, shade in (('none', 'color'), ('back', 'normal')):
            kw = dict(cull=cull, shade=shade)
            a = on_device(v, f, col, K, E, H, W, **kw)
            b = on_device(v, f, col, K, E, H, W, **kw)
            on_device(*other[1:], cull='none', shade='color')
            c = on_device(v, f, col, K, E, H, W, **kw)
            for k in OUTPUTS:
                assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), (label, cull, shade, k)


def test_triangles_that_fill_a_large_image():
    H = W = 1024
    quad = np.array([[-300, -200, 1], [1500, -200, 1], [1500, 1400, 1], [-300, 1400, 1]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    col = cases.vertex_colors(quad)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = on_device(quad, faces, col, cases.EYE_K, cases.EYE_E, H, W)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print('two screen-filling triangles at 1024^2: %.1f ms (first call, workspace allocation included)' % (seconds * 1e3))
    assert seconds < 5.0                    # one lane walking 10^6 samples would still pass: this catches a hang only
    host = raster.rasterize_host(quad, faces, col, cases.EYE_K, cases.EYE_E, H, W)
    assert_same(out, host, 'quad')
    tri = out['tri_id'].cpu().numpy()
    assert np.all(out['alpha'].cpu().numpy() == 1) and set(np.unique(tri)) == {0, 1}
    # split along the diagonal from (-300, -200) to (1500, 1400): v = -200 + (u + 300) 8 / 9; samples on it go to one side
    jj, ii = np.mgrid[0:H, 0:W]
    side = 9 * (jj + 200) - 8 * (ii + 300)
    assert np.all(tri[side < 0] == 0) and np.all(tri[side > 0] == 1)
    assert len(set(tri[side == 0])) == 1 and (side == 0).sum() > 50
    assert np.all(out['depth'].cpu().numpy() == 1)


# ------------------------------------------------------------------------------------------------- through the network
@pytest.fixture(scope='module')
def net():
    state = with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0)
    n = Network()
    n.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return n.to(DEV).eval()


def test_render_mesh_through_the_network(net):
    frame = scene.synthetic_frame(H=64, W=64, pose_seed=3, pose_scale=0.3, camera_only=True)
    verts, faces, colors = net.extract_canonical_mesh(frame['cnl_bbox_min_xyz'], frame['cnl_bbox_max_xyz'],
                                                      frame['motion_weights_priors'], resolution=64, level=LEVEL)
    posed = net.pose_vertices(verts, frame)
    for kw in (dict(), dict(cull='back', shade='normal')):
        out = net.render_mesh(verts, faces, colors, frame, **kw)
        host = raster.rasterize_host(posed.cpu().numpy(), faces.cpu().numpy(), colors.cpu().numpy(), frame['K'], frame['E'],
                                     64, 64, bgcolor=frame['bgcolor'] / 255., **kw)
        assert_same(out, host, kw)
        assert 100 < int((out['tri_id'] >= 0).sum()) < 64 * 64
        again = net.render_mesh(posed, faces, colors, frame, posed=True, **kw)
        for k in OUTPUTS:
            assert torch.equal(out[k], again[k])
    bg = dict(frame, bgcolor=np.array([255., 0., 51.], np.float32))
    out = net.render_mesh(verts, faces, colors, bg)
    assert torch.equal(out['rgb'][out['alpha'] == 0].cpu().unique(dim=0), torch.tensor([[1.0, 0.0, 0.2]]))
    for missing in ('K', 'E'):
        with pytest.raises(HnrfError, match=repr(missing)):
            net.render_mesh(verts, faces, colors, {k: v for k, v in frame.items() if k != missing})
    with pytest.raises(HnrfError, match="'K'"):                        # a host-ray frame has rays, not a camera
        net.render_mesh(verts, faces, colors, scene.synthetic_frame(H=64, W=64, pose_seed=3, pose_scale=0.3))


def test_run_mesh_render_writes_the_three_sequences(net, tmp_path):
    from PIL import Image
    from humannerf_amd import dataset, render, run
    names = scene.write_synthetic_subject(str(tmp_path / 'subject'), n_frames=2, size=64)
    subject = dataset.Subject(str(tmp_path / 'subject'))
    old = cfg.get('show_alpha', False)
    cfg.show_alpha = False
    try:
        log = str(tmp_path / 'log')
        res = {kind: run.run_mesh_render(net, subject, kind=kind, resolution=64, level=LEVEL, logdir=log, total_frames=2,
                                         frame_idx=1, image_size=(64, 64)) for kind in ('movement', 'freeview', 'tpose')}
        for kind, folder, files in (('movement', 'mesh_movement', [n + '.png' for n in names]),
                                    ('freeview', 'mesh_freeview_1', ['000000.png', '000001.png']),
                                    ('tpose', 'mesh_tpose', ['000000.png', '000001.png'])):
            r = res[kind]
            assert os.path.basename(r['image_dir']) == folder and sorted(os.listdir(r['image_dir'])) == files
            assert r['frames'] == [0, 1] and set(r['images']) == {0, 1} and set(r) == {'frames', 'images', 'image_dir', 'stack'}
            for i, fn in enumerate(files):
                im = np.asarray(Image.open(os.path.join(r['image_dir'], fn)))
                assert im.shape == (64, 64, 3) and np.array_equal(im, r['images'][i])
                assert len(np.unique(im.reshape(-1, 3), axis=0)) > 10                  # not all background
            assert not np.array_equal(r['images'][0], r['images'][1])
        # the normal view of the movement loop is the .ply of run_mesh seen through the frame's camera
        nrm = run.run_mesh_render(net, subject, kind='movement', resolution=64, level=LEVEL, logdir=str(tmp_path / 'log2'),
                                  image_size=(64, 64), shade='normal')
        plys = run.run_mesh(net, subject, frames=(0, 1), resolution=64, level=LEVEL, logdir=str(tmp_path / 'log2'))
        for i, n in enumerate(names):
            v, f, _ = mesh.read_ply(plys[n])
            fr = subject.movement_frame(i, image_size=(64, 64))
            host = raster.rasterize_host(v, f, None, fr['K'], fr['E'], 64, 64, bgcolor=fr['bgcolor'] / 255., cull='back',
                                         shade='normal')
            im = np.asarray(Image.open(os.path.join(nrm['image_dir'], n + '.png')))
            assert (host['tri_id'] >= 0).sum() > 100
            assert np.array_equal(im, render.to_8b_image(host['rgb']))
    finally:
        cfg.show_alpha = old


def test_run_mesh_render_with_video(net, tmp_path):
    """cfg.amd.video in the mesh loop, panels [render | alpha]: 'mjpeg' writes an AVI of the 2 frames next to the PNGs,
    each frame the twin's stream of its PNG's pixels, named like the PNGs; 'mjpeg_only' writes no PNG, no directory, and
    the same AVI byte for byte."""
    from PIL import Image
    from humannerf_amd import dataset, run, video
    scene.write_synthetic_subject(str(tmp_path / 'subject'), n_frames=2, size=64)
    subject = dataset.Subject(str(tmp_path / 'subject'))
    old = (cfg.get('show_alpha', False), {k: cfg.amd[k] for k in ('video', 'metrics') if k in cfg.amd})
    cfg.show_alpha = True
    cfg.amd.metrics = 'device'              # (the loop computes none; 'mjpeg_only' is refused next to the host route)
    try:
        res = {}
        for mode in ('mjpeg', 'mjpeg_only'):
            cfg.amd.video = mode
            res[mode] = run.run_mesh_render(net, subject, kind='tpose', total_frames=2, resolution=64, level=LEVEL,
                                            image_size=64, logdir=str(tmp_path / mode))
        both, only = res['mjpeg'], res['mjpeg_only']
        assert both['video'] == both['image_dir'] + '.avi' and sorted(os.listdir(both['image_dir'])) == ['000000.png', '000001.png']
        w, h, fps, frames = video.read_avi(both['video'])
        assert (w, h, fps, len(frames)) == (128, 64, 10, 2)
        for i, data in enumerate(frames):
            pixels = np.asarray(Image.open(os.path.join(both['image_dir'], '%06d.png' % i)))
            assert pixels.shape == (64, 128, 3) and np.array_equal(pixels[:, :64], both['images'][i])
            assert data == video.jpeg_encode_numpy(pixels, 90)
        assert frames[0] != frames[1]
        with open(both['video'] + '.names.txt') as f:
            assert f.read().split() == ['000000', '000001']
        assert only['images'] == {} and only['stack'] is None and not os.path.exists(only['image_dir'])
        assert [f for _, _, fs in os.walk(str(tmp_path / 'mjpeg_only')) for f in fs if f.endswith('.png')] == []
        with open(only['video'], 'rb') as a, open(both['video'], 'rb') as b:
            assert a.read() == b.read()
    finally:
        cfg.show_alpha = old[0]
        for k in ('video', 'metrics'):
            if k in old[1]:
                cfg.amd[k] = old[1][k]
            else:
                cfg.amd.pop(k, None)
