"""The Motion-JPEG path without a GPU (humannerf_amd/video.py, include/hnrf_video.h): the numpy twin of the encoder
against PIL's libjpeg, the slot bound, the AVI container against a RIFF walker of this file's own, the options and the
ABI tables."""
import os
import struct

import numpy as np
import pytest

import video_cases as vc
from humannerf_amd import _lib, video
from humannerf_amd.config import check_amd_options, get_cfg_defaults


# ------------------------------------------------------------------------------------------------ 1, 2: the twin
@pytest.mark.parametrize('name,q', vc.CASES)
def test_twin_stream_decodes(name, q):
    """Every stream opens and fully loads in PIL with warnings as errors; size and quantisation tables are those of
    PIL's own save(quality=q, subsampling=2) of the same image."""
    stream, _ = vc.twin(name, q)
    src = vc.images()[name]
    dec, quant = vc.decode(stream)
    assert dec.shape == src.shape
    _, pil_quant = vc.decode(vc.pil_encode(name, q))
    assert quant == pil_quant
    assert stream[:2] == b'\xff\xd8' and stream[-2:] == b'\xff\xd9'


def test_images_reach_their_paths():
    """The twin's own counters, not trust: what each image is in the set for."""
    c = lambda name, q: vc.twin(name, q)[1]
    big = c('144x48_rect', 100)
    assert big['max_dc_diff'] > 1023 and big['zrl'] > 0 and big['eob_absent'] > 0        # size category 11
    assert c('48x48_noise', 50)['zrl'] > 0
    for q in (90, 100):
        assert c('48x48_noise', q)['eob_absent'] > 27                                     # most of the 54 blocks
    assert c('48x48_noise', 100)['stuffed'] >= 24                                         # dozens
    assert c('16x16_smooth', 50) == {'zrl': 0, 'eob_absent': 0, 'stuffed': 0, 'max_dc_diff': c('16x16_smooth', 50)['max_dc_diff']}
    assert c('528x512_noise', 100)['stuffed'] > 1000
    # RST markers: 27 MCUs -> RST0 .. RST7 three times and RST0, RST1; one MCU -> none
    s = vc.twin('144x48_rect', 50)[0]
    body = s[len(video.jpeg_header(48, 144, 50)):]
    rst = [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xFF and 0xD0 <= body[i + 1] <= 0xD7]
    assert rst == [0xD0 + (i & 7) for i in range(26)]
    one = vc.twin('16x16_smooth', 50)[0][len(video.jpeg_header(16, 16, 50)):]
    assert not any(one[i] == 0xFF and 0xD0 <= one[i + 1] <= 0xD7 for i in range(len(one) - 1))


@pytest.mark.parametrize('name,q', [(n, q) for n, q in vc.CASES if q != 100])
def test_twin_psnr_not_below_pil(name, q):
    """Decoded PSNR against the source >= PIL's own encode at the same q minus vc.PSNR_MARGIN_DB (measured shortfall
    0.159 dB, doubled).  q = 100 is left out: there the rounding of the colour transform dominates either way."""
    src = vc.images()[name]
    mine = vc.psnr(vc.decode(vc.twin(name, q)[0])[0], src)
    pil = vc.psnr(vc.decode(vc.pil_encode(name, q))[0], src)
    print('%s q=%d: twin %.3f dB, PIL %.3f dB, shortfall %.3f dB' % (name, q, mine, pil, pil - mine))
    assert mine >= pil - vc.PSNR_MARGIN_DB


def test_twin_speed_and_counters_arg():
    import time
    t0 = time.perf_counter()
    video.jpeg_encode_numpy(vc.images()['528x512_noise'], 90)
    assert time.perf_counter() - t0 < 5.0            # "a few seconds": measured 0.15 s


def test_twin_refuses_bad_input():
    with pytest.raises(ValueError):
        video.jpeg_encode_numpy(np.zeros((4, 4, 3), dtype=np.uint8), 0)
    with pytest.raises(ValueError):
        video.jpeg_encode_numpy(np.zeros((4, 4, 3), dtype=np.uint8), 101)
    with pytest.raises(ValueError):
        video.jpeg_encode_numpy(np.zeros((0, 4, 3), dtype=np.uint8), 50)
    with pytest.raises(ValueError):
        video.jpeg_encode_numpy(np.zeros((4, 4, 3), dtype=np.float32), 50)


# ------------------------------------------------------------------------------------------------ 3: the slot bound
def test_slot_bound():
    """The constant is the derived bound, and adversarial MCUs (maximal-amplitude checkerboard-like content at
    q = 100: every coefficient large, so every code long) stay inside it."""
    assert video.slot_bound() == video.SLOT_BYTES == 2 * 1244 + 8
    with open(_lib.VIDEO_HEADER_PATH) as f:
        assert '#define HNRF_JPEG_SLOT_BYTES %d\n' % video.SLOT_BYTES in f.read()
    rs = np.random.RandomState(7)
    blocks = []
    for i in range(300):
        kind = i % 3
        if kind == 0:                                # per-pixel black / white noise, channels independent
            b = rs.randint(0, 2, (16, 16, 3)) * 255
        elif kind == 1:                              # a checkerboard with a few cells flipped
            y, x = np.mgrid[0:16, 0:16]
            b = (((x + y) & 1) * 255)[..., None].repeat(3, 2)
            flip = rs.rand(16, 16) < 0.15
            b[flip] = 255 - b[flip]
        else:                                        # saturated primaries per pixel: large chroma as well
            b = np.eye(3, dtype=np.int64)[rs.randint(0, 3, (16, 16))] * 255
        blocks.append(b.astype(np.uint8))
    img = np.concatenate(blocks, axis=1)             # 300 MCUs side by side
    mcus, _ = video.encode_mcus(video.mcu_coefficients(img, 100))
    longest = max(len(m) for m in mcus)
    print('longest adversarial MCU: %d bytes of %d' % (longest, video.SLOT_BYTES))
    assert 500 < longest <= video.SLOT_BYTES         # (the search does reach long streams: 608 bytes)


# ------------------------------------------------------------------------------------------------ 4: the container
def _walk(data, pos, end, out, path=()):
    """Every chunk between pos and end as (path, fourcc, data offset, size); LISTs are descended into."""
    while pos < end:
        assert pos + 8 <= end, 'a chunk header runs past its parent'
        cc, size = data[pos:pos + 4], struct.unpack('<I', data[pos + 4:pos + 8])[0]
        assert pos + 8 + size <= end, 'a chunk runs past its parent'
        if cc == b'LIST':
            kind = data[pos + 8:pos + 12]
            out.append((path, b'LIST:' + kind, pos + 8, size))
            _walk(data, pos + 12, pos + 8 + size, out, path + (kind,))
        else:
            out.append((path, cc, pos + 8, size))
        pos += 8 + size + (size & 1)
        if size & 1:
            assert data[pos - 1] == 0
    assert pos == end, 'sizes and padding do not add up'


def _riff(data):
    assert data[:4] == b'RIFF' and data[8:12] == b'AVI '
    assert struct.unpack('<I', data[4:8])[0] + 8 == len(data)
    out = []
    _walk(data, 12, len(data), out)
    return out


def _frames_for_container():
    """Five frames of one size added out of name order, three of odd and two of even length (chunk padding)."""
    names = ['frame_%06d' % i for i in (3, 0, 4, 1, 2)]
    cand = [video.jpeg_encode_numpy(vc.images()['40x24'], q) for q in range(40, 72, 2)]
    odd, even = [c for c in cand if len(c) & 1], [c for c in cand if not len(c) & 1]
    picked = odd[:3] + even[:2]
    assert len(picked) == 5 and len(set(picked)) == 5
    return names, dict(zip(names, [picked[0], picked[3], picked[1], picked[4], picked[2]]))


def test_mjpeg_writer_against_riff_walker(tmp_path):
    names, streams = _frames_for_container()
    assert len({len(s) & 1 for s in streams.values()}) == 2, 'the frames should cover odd and even lengths'
    path = str(tmp_path / 'out' / 'clip.avi')
    w = video.MjpegWriter(path, 40, 24, fps=10)
    for n in names:
        w.add(n, streams[n])
    assert w.finalize() == path
    data = open(path, 'rb').read()
    chunks = _riff(data)
    kinds = [(p, c) for p, c, _, _ in chunks]
    assert kinds[:6] == [((), b'LIST:hdrl'), ((b'hdrl',), b'avih'), ((b'hdrl',), b'LIST:strl'), ((b'hdrl', b'strl'), b'strh'),
                         ((b'hdrl', b'strl'), b'strf'), ((), b'LIST:movi')]
    assert kinds[6:-1] == [((b'movi',), b'00dc')] * 5 and kinds[-1] == ((), b'idx1')
    get = lambda cc: [(o, s) for _, c, o, s in chunks if c == cc]
    (o, s), = get(b'avih')
    avih = struct.unpack('<14I', data[o:o + s])
    assert avih[0] == 100000 and avih[4] == 5 and avih[6] == 1 and avih[8:10] == (40, 24) and avih[3] & 0x10
    (o, s), = get(b'strh')
    assert data[o:o + 8] == b'vidsMJPG'
    scale, rate, _, length = struct.unpack('<4I', data[o + 20:o + 36])
    assert rate / scale == 10 and length == 5
    (o, s), = get(b'strf')
    bih = struct.unpack('<IiiHH4sIiiII', data[o:o + s])
    assert bih[0] == 40 == s and bih[1:3] == (40, 24) and bih[3] == 1 and bih[4] == 24 and bih[5] == b'MJPG'
    movi_data, _ = get(b'LIST:movi')[0]
    frames = get(b'00dc')
    for (o, s), n in zip(frames, sorted(names)):                 # sorted by name, bytes as added, decodable
        assert data[o:o + s] == streams[n]
        assert vc.decode(data[o:o + s])[0].shape == (24, 40, 3)
    (o, s), = get(b'idx1')
    assert s == 16 * 5
    for k in range(5):
        cc, flags, off, size = struct.unpack('<4sIII', data[o + 16 * k:o + 16 * k + 16])
        at = movi_data + off                                     # offsets count from the 'movi' fourcc
        assert cc == b'00dc' and flags & 0x10
        assert data[at:at + 4] == b'00dc' and struct.unpack('<I', data[at + 4:at + 8])[0] == size == frames[k][1]
        assert at + 8 == frames[k][0]
    assert open(path + '.names.txt').read().split('\n') == sorted(names) + ['']


def test_merge_parts_equals_one_file(tmp_path):
    names, streams = _frames_for_container()
    whole = video.MjpegWriter(str(tmp_path / 'whole.avi'), 40, 24, fps=10)
    parts = [video.MjpegWriter(str(tmp_path / ('clip.rank%d.avi' % r)), 40, 24, fps=10) for r in range(2)]
    for i, n in enumerate(sorted(names)):
        whole.add(n, streams[n])
        parts[i % 2].add(n, streams[n])                          # frame-sharded: rank r has frames r, r + 2, ...
    whole.finalize()
    paths = [p.finalize() for p in parts]
    merged = video.merge_parts(paths, str(tmp_path / 'merged.avi'))
    assert open(merged, 'rb').read() == open(str(tmp_path / 'whole.avi'), 'rb').read()
    assert open(merged + '.names.txt').read() == open(str(tmp_path / 'whole.avi.names.txt')).read()


def test_mjpeg_writer_refusals(tmp_path, monkeypatch):
    with pytest.raises(ValueError):
        video.MjpegWriter(str(tmp_path / 'a.avi'), 40, 24, fps=0)
    w = video.MjpegWriter(str(tmp_path / 'a.avi'), 40, 24)
    assert w.fps == 10
    w.add('a', b'\xff\xd8\xff\xd9')
    with pytest.raises(ValueError):
        w.add('a', b'\xff\xd8\xff\xd9')
    monkeypatch.setattr(video, 'RIFF_LIMIT', 100)                # the 2 GiB rule at a size a test can reach
    with pytest.raises(ValueError, match='a.avi'):
        w.finalize()
    assert not os.path.exists(str(tmp_path / 'a.avi'))


# ------------------------------------------------------------------------------------------------ 5: options
def test_check_amd_options_video():
    node = dict(get_cfg_defaults().amd)
    assert (node['video'], node['video_quality'], node['video_fps']) == ('none', 90, 10)
    check_amd_options(node)
    for ok in ({'video': 'mjpeg'}, {'video': 'mjpeg', 'video_quality': 1, 'video_fps': 30},
               {'video': 'mjpeg_only', 'metrics': 'device', 'video_quality': 100}):
        check_amd_options(dict(node, **ok))
    for bad in ({'video': 'mp4'}, {'video': True}, {'video_quality': 0}, {'video_quality': 101}, {'video_quality': 90.0},
                {'video_quality': True}, {'video_fps': 0}, {'video_fps': 2.5}, {'video_fps': '10'}):
        with pytest.raises(ValueError):
            check_amd_options(dict(node, **bad))
    with pytest.raises(ValueError, match='mjpeg_only'):
        check_amd_options(dict(node, video='mjpeg_only', metrics='host'))


# ------------------------------------------------------------------------------------------------ 6: the ABI
VIDEO_SYMBOLS = ['hnrf_jpeg_encode', 'hnrf_jpeg_header', 'hnrf_jpeg_max_bytes', 'hnrf_jpeg_workspace_bytes']


def _built():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def test_video_signatures_and_exports():
    import ctypes
    assert sorted(_lib.VIDEO_SIGNATURES) == VIDEO_SYMBOLS
    assert not set(_lib.VIDEO_SIGNATURES) & set(_lib.SIGNATURES)
    assert not set(_lib.VIDEO_SIGNATURES) & set(_lib.CLOUD_SIGNATURES)
    res, args = _lib.VIDEO_SIGNATURES['hnrf_jpeg_encode']
    assert res is ctypes.c_int and len(args) == 13 and args[3] is ctypes.c_int64 and args[8] is ctypes.c_size_t
    assert _lib.VIDEO_SIGNATURES['hnrf_jpeg_max_bytes'] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    _built()
    lib = _lib.load_video()                      # raises when the library lacks one of them
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in VIDEO_SYMBOLS:
        assert getattr(raw, name) is not None
    assert lib.hnrf_abi_version() == 13


def test_host_entries_without_a_gpu():
    """hnrf_jpeg_header runs on the host: the bytes of the twin's header; the size functions and their refusals."""
    import ctypes
    _built()
    lib = _lib.load_video()
    buf = (ctypes.c_uint8 * 1024)()
    for H, W, q in ((1, 1, 10), (512, 528, 90), (65535, 3, 100), (33, 17, 50)):
        n = lib.hnrf_jpeg_header(H, W, q, buf, 1024)
        assert bytes(buf[:n]) == video.jpeg_header(H, W, q)
    for H, W, q, cap in ((0, 1, 50, 1024), (1, 65536, 50, 1024), (1, 1, 0, 1024), (1, 1, 101, 1024), (1, 1, 50, 100)):
        assert lib.hnrf_jpeg_header(H, W, q, buf, cap) < 0 and b'hnrf_jpeg_header' in lib.hnrf_last_error()
    n_mcu = 33 * 32
    assert lib.hnrf_jpeg_max_bytes(512, 528) == video.HEADER_MAX + n_mcu * (video.SLOT_BYTES + 2)
    assert lib.hnrf_jpeg_workspace_bytes(512, 528) >= n_mcu * (video.SLOT_BYTES + 8)
    assert lib.hnrf_jpeg_max_bytes(0, 5) == 0 and lib.hnrf_jpeg_workspace_bytes(5, 65536) == 0


# ------------------------------------------------------------------------------------------------ the loop on a CPU device
def test_render_frames_video_on_a_cpu_device():
    """render_frames(video=...) with a stand-in network on the CPU (the twin encodes): on_video follows on_image frame
    by frame with the stream of exactly the panels run._panels builds; images='none' calls no on_image and returns {}."""
    import torch
    from humannerf_amd import render, run
    from humannerf_amd.config import cfg
    H, W = 24, 40

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

        def forward(self, rays=None, **kw):
            g = torch.Generator().manual_seed(rays.shape[1])
            return {'rgb': torch.rand(rays.shape[1], 3, generator=g), 'alpha': torch.rand(rays.shape[1], generator=g)}

    rs = np.random.RandomState(0)
    frames = []
    for _ in range(3):
        mask = rs.rand(H * W) < 0.6
        n = int(mask.sum())
        fr = {'rays': rs.rand(2, n, 3).astype('f4'), 'near': np.ones(n, 'f4'), 'far': np.ones(n, 'f4'), 'ray_mask': mask,
              'img_width': W, 'img_height': H, 'target_rgbs': rs.rand(n, 3).astype('f4'),
              'motion_weights_priors': np.zeros(3, 'f4'), 'bgcolor': np.array([30., 120., 250.], 'f4')}
        for k in ('dst_Rs', 'dst_Ts', 'cnl_gtfms', 'dst_posevec', 'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz'):
            fr[k] = np.zeros(3, 'f4')
        frames.append(fr)
    old = (cfg.get('show_truth', False), cfg.get('show_alpha', False))
    cfg.show_truth, cfg.show_alpha = True, True
    try:
        dev = torch.device('cpu')
        enc = video.JpegEncoder(dev, 90)
        events, imgs, vids = [], {}, {}
        out = render.render_frames(Net(), frames, device=dev, show_truth=True, video=enc,
                                   on_image=lambda i, *a: (events.append(('image', i)), imgs.__setitem__(i, a)),
                                   on_video=lambda i, d: (events.append(('video', i)), vids.__setitem__(i, d)))
        assert events == [(k, i) for i in range(3) for k in ('image', 'video')] and sorted(out) == [0, 1, 2]
        for i in range(3):
            rgb8, alpha8, truth8 = imgs[i]
            assert vids[i] == video.jpeg_encode_numpy(run._panels(rgb8, alpha8, truth8), 90)
            assert vc.decode(vids[i])[0].shape == (H, 3 * W, 3)
        assert render.render_frames.last_video['frames'] == 3 and render.render_frames.last_video['fallbacks'] == 0
        only = {}
        out = render.render_frames(Net(), frames, device=dev, show_truth=True, video=enc, images='none',
                                   on_image=lambda *a: pytest.fail('on_image with images = none'), on_video=only.__setitem__)
        assert out == {} and only == vids
        with pytest.raises(ValueError, match='none'):
            render.render_frames(Net(), frames, device=dev, images='none')
        with pytest.raises(ValueError):
            render.render_frames(Net(), frames, device=dev, images='gpu', video=enc)
    finally:
        cfg.show_truth, cfg.show_alpha = old


def _outbox_case():
    """A CPU-device FrameOutbox and one frame's products: three 24 x 40 images, a 3-element float64 vector, the twin's
    stream of the images side by side in a buffer longer than the stream (as the encoder's is), and post()'s video tuple."""
    import torch
    from humannerf_amd import render
    rs = np.random.RandomState(5)
    imgs = [rs.randint(0, 256, (24, 40, 3)).astype(np.uint8) for _ in range(3)]
    vals = np.array([31.25, 0.875, 1e-3 / 3], np.float64)
    data = video.jpeg_encode_numpy(np.concatenate(imgs, axis=1), 90)
    vid = (torch.frombuffer(bytearray(data + bytes(100)), dtype=torch.uint8), torch.tensor([len(data)], dtype=torch.int64),
           24, 3 * 40)
    tensors = [torch.from_numpy(im.copy()) for im in imgs]
    return render.FrameOutbox(torch.device('cpu')), imgs, tensors, vals, data, vid


def test_frame_outbox_returns_what_was_posted():
    import torch
    outbox, imgs, tensors, vals, data, vid = _outbox_case()
    parcel = outbox.post(tensors, torch.from_numpy(vals.copy()), vid)
    assert parcel.landed()
    arrs, values, stream, fell_back = parcel.collect()
    assert len(arrs) == 3 and all(a.dtype == np.uint8 and np.array_equal(a, im) for a, im in zip(arrs, imgs))
    assert values == vals.tolist() and stream == data and fell_back is False


def test_frame_outbox_images_only():
    outbox, imgs, tensors, _, _, _ = _outbox_case()
    arrs, values, stream, fell_back = outbox.post(tensors).collect()
    assert len(arrs) == 3 and all(np.array_equal(a, im) for a, im in zip(arrs, imgs))
    assert values is None and stream is None and fell_back is False


def test_frame_outbox_video_only():
    """As render_frames(images='none') posts a frame: no images come back, the whole stream does."""
    outbox, _, _, _, data, vid = _outbox_case()
    arrs, values, stream, fell_back = outbox.post([], video=vid).collect()
    assert arrs == [] and values is None and stream == data and fell_back is False


def test_rank_files_of_a_sharded_loop_merge_into_one(tmp_path):
    """run._VideoOut, the loops' side of cfg.amd.video: with world > 1 rank r writes <folder>.rank<r>.avi with its own
    frames (r, r + world, ...), unnamed frames are called by their index, and merge_parts of the ranks' files is the file
    a single rank writes."""
    import torch
    from humannerf_amd import run
    from humannerf_amd.config import cfg
    old = {k: cfg.amd[k] for k in ('video', 'video_quality', 'video_fps', 'metrics') if k in cfg.amd}
    cfg.amd.video, cfg.amd.video_quality, cfg.amd.video_fps = 'mjpeg', 50, 12
    try:
        dev = torch.device('cpu')
        imgs = [np.ascontiguousarray(np.roll(vc.images()['40x24'], 3 * i, axis=1)) for i in range(5)]
        names = [None] * 5
        paths = []
        for r in range(2):
            v = run._VideoOut(str(tmp_path / 'sharded' / 'freeview_0'), names, r, 2, dev)
            assert v.mode == 'mjpeg' and not v.only and v.encoder.quality == 50
            for i in range(r, 5, 2):
                buf, n = v.encoder.encode(torch.from_numpy(imgs[i]))
                v.add(i, buf[:int(n)].numpy().tobytes())
            paths.append(v.finalize())
        assert [os.path.basename(p) for p in paths] == ['freeview_0.rank0.avi', 'freeview_0.rank1.avi']
        one = run._VideoOut(str(tmp_path / 'single' / 'freeview_0'), names, 0, 1, dev)
        for i in range(5):
            one.add(i, video.jpeg_encode_numpy(imgs[i], 50))
        whole = one.finalize()
        assert os.path.basename(whole) == 'freeview_0.avi'
        merged = video.merge_parts(paths, str(tmp_path / 'merged.avi'))
        assert open(merged, 'rb').read() == open(whole, 'rb').read()
        w, h, fps, frames = video.read_avi(merged)
        assert (w, h, fps, len(frames)) == (40, 24, 12, 5)
        assert open(merged + '.names.txt').read().split() == ['%06d' % i for i in range(5)]
        cfg.amd.video = 'none'
        off = run._VideoOut(str(tmp_path / 'off'), names, 0, 1, dev)
        assert off.encoder is None and not off.only and off.finalize() is None
    finally:
        for k in ('video', 'video_quality', 'video_fps', 'metrics'):
            if k in old:
                cfg.amd[k] = old[k]
            else:
                cfg.amd.pop(k, None)
