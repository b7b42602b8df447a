"""The JPEG encoder on the MI355X (csrc/hnrf_video.hip through humannerf_amd/video.py) against its numpy twin, byte for
byte, and the Motion-JPEG option of the render loops."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import video_cases as vc
from humannerf_amd import _lib, video

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def encoders():
    return {q: video.JpegEncoder(DEV, q) for q in vc.QUALITIES}


def _stream(enc, t):
    buf, n = enc.encode(t)
    n = int(n.item())
    return bytes(buf[:n].cpu().numpy().tobytes())


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize('name,q', vc.CASES)
def test_device_stream_equals_twin(name, q, encoders):
    got = _stream(encoders[q], torch.from_numpy(vc.images()[name].copy()).to(DEV))
    want = vc.twin(name, q)[0]
    assert len(got) == len(want)
    assert got == want


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('name', ['40x24', '17x33_bw', '144x48_rect'])
def test_row_stride(name, encoders):
    """A column slice of a wider tensor goes through row_stride (no copy: the slice's stride is handed over) and gives
    the bytes of its contiguous copy."""
    img = vc.images()[name]
    H, W = img.shape[:2]
    wide = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (H, W + 21, 3)).astype(np.uint8)).to(DEV)
    wide[:, 5:5 + W] = torch.from_numpy(img.copy()).to(DEV)
    view = wide[:, 5:5 + W]
    assert not view.is_contiguous() and view.stride(0) == 3 * (W + 21)
    assert _stream(encoders[90], view) == _stream(encoders[90], view.contiguous()) == vc.twin(name, 90)[0]


# ------------------------------------------------------------------------------------------------ 3
def _raw_encode(lib, img_t, q, ws, ws_bytes, out, out_cap, length):
    H, W = img_t.shape[:2]
    host = (ctypes.c_uint8 * 1024)()
    n = lib.hnrf_jpeg_header(H, W, q, host, 1024)
    header = torch.frombuffer(bytearray(host)[:n], dtype=torch.uint8).to(DEV)
    rc = lib.hnrf_jpeg_encode(img_t.data_ptr(), H, W, 3 * W, header.data_ptr(), n, q, ws.data_ptr(), ws_bytes, out.data_ptr(),
                              out_cap, length.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_bounds_and_workspace_reuse():
    """out and the workspace carry a 4 KB tail of a pattern: the tail and everything past out_len stay untouched; the
    same image encoded twice, with another image through the same workspace in between, gives the same bytes."""
    lib = _lib.load_video()
    a = torch.from_numpy(vc.images()['144x48_rect'].copy()).to(DEV)
    b = torch.from_numpy(np.ascontiguousarray(vc.images()['528x512_noise'][:48, :144])).to(DEV)
    H, W, q = 48, 144, 100
    ws_bytes, cap = int(lib.hnrf_jpeg_workspace_bytes(H, W)), int(lib.hnrf_jpeg_max_bytes(H, W))
    ws = torch.full((ws_bytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    results = []
    for img in (a, b, a):
        out = torch.full((cap + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
        length = torch.zeros(1, dtype=torch.int64, device=DEV)
        assert _raw_encode(lib, img, q, ws, ws_bytes, out, cap, length) == 0
        n = int(length.item())
        assert 613 < n <= cap
        assert bool((out[n:] == 0x5A).all()), 'bytes past out_len were written'
        assert bool((ws[ws_bytes:] == 0xA5).all()), 'the tail of the workspace was written'
        results.append(out[:n].cpu().numpy().tobytes())
    assert results[0] == results[2] == vc.twin('144x48_rect', q)[0]
    assert results[1] != results[0]


# ------------------------------------------------------------------------------------------------ 4
def test_refusals_launch_nothing():
    lib = _lib.load_video()
    img = torch.from_numpy(vc.images()['40x24'].copy()).to(DEV)
    H, W = 24, 40
    ws_bytes, cap = int(lib.hnrf_jpeg_workspace_bytes(H, W)), int(lib.hnrf_jpeg_max_bytes(H, W))
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((cap,), 0x5A, dtype=torch.uint8, device=DEV)
    length = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    header = torch.zeros(613, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(H=H, W=W, q=90, cap=cap, ws_bytes=ws_bytes, stride=3 * W):
        return lib.hnrf_jpeg_encode(img.data_ptr(), H, W, stride, header.data_ptr(), 613, q, ws.data_ptr(), ws_bytes,
                                    out.data_ptr(), cap, length.data_ptr(), st)

    for kw in (dict(H=0), dict(W=0), dict(W=65536), dict(q=0), dict(q=101), dict(cap=cap - 1), dict(ws_bytes=ws_bytes - 1),
               dict(stride=3 * W - 1)):
        assert call(**kw) != 0, kw
        msg = lib.hnrf_last_error()
        assert msg and b'hnrf_jpeg_encode' in msg, kw
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and bool((ws == 0xA5).all()) and int(length.item()) == -1
    with pytest.raises(ValueError):
        video.JpegEncoder(DEV, 0)
    with pytest.raises(ValueError):
        video.JpegEncoder(DEV, 90).encode(torch.zeros(4, 4, 3, device=DEV))


# ------------------------------------------------------------------------------------------------ 5: the copy-out
def _products(seed):
    """One frame's host-bound products on the device: three 8 x 8 images, a float64 vector, a made-up 2000-byte stream
    in a 3000-byte buffer with its length word."""
    rs = np.random.RandomState(seed)
    imgs = [rs.randint(0, 256, (8, 8, 3)).astype(np.uint8) for _ in range(3)]
    vals = rs.rand(3)
    stream = rs.randint(0, 256, 3000).astype(np.uint8)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    return imgs, vals, stream[:2000].tobytes(), ([dev(im) for im in imgs], dev(vals),
                                                 (dev(stream), torch.tensor([2000], dtype=torch.int64, device=DEV), 8, 24))


def test_frame_outbox_round_trip(monkeypatch):
    """Three parcels in flight at once come back as posted; the real cap (>= 64 KiB) covers the stream, a cap of 700
    makes every collect() fetch the remainder and still return all 2000 bytes."""
    from humannerf_amd import render
    outbox = render.FrameOutbox(DEV)
    for cap, falls_back in ((None, False), (700, True)):
        if cap is not None:
            monkeypatch.setattr(render, 'video_copy_cap', lambda height, width: cap)
        want = [_products(seed) for seed in range(3)]
        parcels = [outbox.post(*w[3]) for w in want]
        assert [p.cap for p in parcels] == [3000 if cap is None else cap] * 3
        for (imgs, vals, data, _), parcel in zip(want, parcels):
            arrs, values, stream, fell_back = parcel.collect()
            assert len(arrs) == 3 and all(np.array_equal(a, im) for a, im in zip(arrs, imgs))
            assert values == vals.tolist() and len(stream) == 2000 and stream == data and fell_back is falls_back


def test_frame_outbox_reuses_its_pinned_buffers():
    """post, collect, post of the same shapes: the second parcel's pinned buffers are the first one's -- they went back
    to the pool; the same after discard(), which the re-render after an f16-range hit relies on."""
    from humannerf_amd import render
    outbox = render.FrameOutbox(DEV)
    ptrs = lambda parcel: sorted(h.data_ptr() for h in parcel.buffers())
    first = outbox.post(*_products(0)[3])
    mine = ptrs(first)
    assert len(set(mine)) == 6 and all(h.is_pinned() for h in first.buffers())       # 3 images, vector, stream, length
    first.collect()
    second = outbox.post(*_products(1)[3])
    assert ptrs(second) == mine
    second.discard()
    third = outbox.post(*_products(2)[3])
    assert ptrs(third) == mine
    imgs, vals, data, _ = _products(2)
    arrs, values, stream, _ = third.collect()
    assert all(np.array_equal(a, im) for a, im in zip(arrs, imgs)) and values == vals.tolist() and stream == data


# ------------------------------------------------------------------------------------------------ 6: the loops
def _seeded_net(scale=None):
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state, with_density
    n = Network()
    n.load_state_dict({k: torch.from_numpy(v) for k, v in with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0).items()})
    n = n.to(DEV).eval()
    if scale is not None:                            # the out-of-range checkpoint of tests/test_gpu_parity.py
        with torch.no_grad():
            n.state_dict()[scale].mul_(3.0e5)
    return n


@pytest.fixture(scope='module')
def net():
    return _seeded_net()


@pytest.fixture()
def loop_cfg():
    from humannerf_amd.config import cfg
    amd = cfg.amd
    keys = ('metrics', 'video', 'video_quality', 'video_fps', 'on_f16_range')
    old = (cfg.get('show_truth', False), cfg.get('show_alpha', False), amd.diagnostics, cfg.N_samples,
           {k: amd[k] for k in keys if k in amd})
    amd.diagnostics, cfg.N_samples, cfg.show_alpha = False, 64, True
    yield cfg
    cfg.show_truth, cfg.show_alpha, amd.diagnostics, cfg.N_samples = old[:4]
    for k in keys:
        if k in old[4]:
            amd[k] = old[4][k]
        else:
            amd.pop(k, None)


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def _movement(net, subject, logdir, mode, route='host'):
    from humannerf_amd import run
    from humannerf_amd.config import cfg
    cfg.amd.video, cfg.amd.metrics = mode, route
    res = run.run_movement(net, subject, logdir=logdir, metrics=['psnr', 'ssim'])
    base = res['image_dir'].rstrip('/')
    pngs = {f: _read(os.path.join(base, f)) for f in sorted(os.listdir(base)) if f.endswith('.png')} if os.path.isdir(base) else None
    texts = (_read(base + '-metrics.perimg.txt'), _read(base + '-metrics.average.txt'))
    return res, pngs, texts


def test_run_movement_writes_the_video(net, tmp_path, loop_cfg):
    """3-frame synthetic subject, 64 x 64, panels [render | truth | alpha]: 'mjpeg' leaves the PNGs of 'none' byte for
    byte and an AVI of 3 frames in name order, each the twin's stream of that frame's PNG pixels (so decodable, of the
    panel's size, and within the PSNR margin of PIL's own encode); 'mjpeg_only' writes no PNG and the same AVI; the
    metric files of the device route are the same in all three modes."""
    import io
    from PIL import Image
    from humannerf_amd import dataset, render, scene
    names = scene.write_synthetic_subject(str(tmp_path / 'subject'), n_frames=3, size=64)
    subject = dataset.Subject(str(tmp_path / 'subject'))
    none, png0, txt0 = _movement(net, subject, str(tmp_path / 'none'), 'none', 'device')
    assert 'video' not in none and not glob.glob(str(tmp_path / 'none' / '**' / '*.avi'), recursive=True)
    both, png1, txt1 = _movement(net, subject, str(tmp_path / 'mjpeg'), 'mjpeg', 'device')
    assert png1 == png0 and list(png0) == sorted(n + '.png' for n in names)
    assert txt1 == txt0
    assert both['video'] == both['image_dir'].rstrip('/') + '.avi' and os.path.isfile(both['video'])
    w, h, fps, frames = video.read_avi(both['video'])
    assert (w, h, fps, len(frames)) == (3 * 64, 64, 10, 3)
    assert _read(both['video'] + '.names.txt').decode().split() == sorted(names)
    assert render.render_frames.last_video['frames'] == 3 and render.render_frames.last_video['fallbacks'] == 0
    for name, data in zip(sorted(names), frames):
        pixels = np.asarray(Image.open(io.BytesIO(png0[name + '.png'])))
        assert pixels.shape == (64, 3 * 64, 3)
        dec, _ = vc.decode(data)
        assert dec.shape == pixels.shape
        mine = vc.psnr(dec, pixels)
        pil = vc.psnr(vc.decode(vc.pil_encode_array(pixels, 90))[0], pixels)
        print('%s: %d bytes, PSNR %.3f dB, PIL %.3f dB' % (name, len(data), mine, pil))
        assert mine >= pil - vc.PSNR_MARGIN_DB
        assert data == video.jpeg_encode_numpy(pixels, 90)               # the device encoded exactly these panels
    only, png2, txt2 = _movement(net, subject, str(tmp_path / 'only'), 'mjpeg_only', 'device')
    assert png2 is None or png2 == {}
    assert not glob.glob(str(tmp_path / 'only' / '**' / '*.png'), recursive=True)
    assert not glob.glob(str(tmp_path / 'only' / '**' / '*.npy'), recursive=True)
    assert only['images'] == {} and _read(only['video']) == _read(both['video'])
    assert txt2 == txt0
    # host metrics with the PNGs still there: the same files as without the video
    hnone, _, htxt0 = _movement(net, subject, str(tmp_path / 'hnone'), 'none', 'host')
    hboth, hpng, htxt1 = _movement(net, subject, str(tmp_path / 'hmjpeg'), 'mjpeg', 'host')
    assert htxt1 == htxt0 and hpng == png0 and _read(hboth['video']) == _read(both['video'])
    loop_cfg.amd.video, loop_cfg.amd.metrics = 'mjpeg_only', 'host'
    from humannerf_amd import run
    with pytest.raises(ValueError, match='mjpeg_only'):
        run.run_movement(net, subject, logdir=str(tmp_path / 'refused'), metrics=['psnr'])


def test_freeview_and_quality_and_fps(net, tmp_path, loop_cfg, monkeypatch):
    """Unnamed frames (freeview: %06d like the PNGs), one panel wide without show_alpha, video_quality and video_fps;
    and with a copy cap below the streams' length every frame takes the fall-back and arrives whole."""
    from humannerf_amd import dataset, render, run, scene
    scene.write_synthetic_subject(str(tmp_path / 'subject'), n_frames=3, size=64)
    subject = dataset.Subject(str(tmp_path / 'subject'))
    loop_cfg.show_alpha = False
    loop_cfg.amd.video, loop_cfg.amd.video_quality, loop_cfg.amd.video_fps = 'mjpeg', 50, 25
    res = run.run_freeview(net, subject, frame_idx=1, total_frames=3, logdir=str(tmp_path / 'fv'))
    w, h, fps, frames = video.read_avi(res['video'])
    assert (w, h, fps, len(frames)) == (64, 64, 25, 3)
    assert _read(res['video'] + '.names.txt').decode().split() == ['%06d' % i for i in range(3)]
    for i, data in enumerate(frames):
        assert data == video.jpeg_encode_numpy(res['images'][i], 50)
    # (the cap is the smaller of video_copy_cap and the buffer: 16 MCUs' worst case is below the 64 KiB floor)
    assert render.render_frames.last_video['fallbacks'] == 0
    assert render.render_frames.last_video['cap'] == min(64 << 10, video.HEADER_MAX + 16 * (video.SLOT_BYTES + 2))
    monkeypatch.setattr(render, 'video_copy_cap', lambda height, width: 700)
    short = run.run_freeview(net, subject, frame_idx=1, total_frames=3, logdir=str(tmp_path / 'short'))
    assert render.render_frames.last_video['fallbacks'] == 3 and min(len(f) for f in frames) > 700
    assert _read(short['video']) == _read(res['video'])


def test_f16_range_hit_renders_and_encodes_again(tmp_path, loop_cfg):
    """cfg.amd.on_f16_range = 'f32' with the out-of-range checkpoint: the loop terminates, the frames rendered again
    are encoded again, and the file holds exactly the 3 frames -- the streams of the PNGs that were written."""
    import io
    from PIL import Image
    from humannerf_amd import dataset, run, scene
    bad = _seeded_net('cnl_mlp.module.pts_linears.2.weight')
    names = scene.write_synthetic_subject(str(tmp_path / 'subject'), n_frames=3, size=64)
    subject = dataset.Subject(str(tmp_path / 'subject'))
    loop_cfg.amd.on_f16_range, loop_cfg.amd.video, loop_cfg.amd.metrics = 'f32', 'mjpeg', 'host'
    with pytest.warns(UserWarning, match="switching this network to 'f32'"):
        res = run.run_movement(bad, subject, logdir=str(tmp_path / 'log'), metrics=['psnr'])
    assert bad.f16_range_hits >= 1
    w, h, fps, frames = video.read_avi(res['video'])
    assert len(frames) == 3 and _read(res['video'] + '.names.txt').decode().split() == sorted(names)
    for name, data in zip(sorted(names), frames):
        pixels = np.asarray(Image.open(os.path.join(res['image_dir'], name + '.png')))
        assert data == video.jpeg_encode_numpy(pixels, 90)
