"""PSNR / SSIM on the MI355X: ops.image_metrics (hnrf_image_metrics) against its numpy twin render.metrics_u8 --
itself held to render.ssim / render.psnr by tests/test_metrics_cpu.py --, the shapes at which the 32x32 tiling of
window positions can go wrong, reproducibility, no synchronisation, and the device route of render.render_frames /
run.run_movement (cfg.amd.metrics = 'device') against the host route.

Bounds of kernel against twin: a window's value has the same bits on both sides (same integer moments, same fp64
expression without contraction); the sums over the windows are taken in different orders (kernel: 4 rows per lane, a
tree over the lanes, the tiles in order; numpy: pairwise), each good to a few ulp of a mean of values in [-1, 1]:
SSIM within 1e-12.  PSNR: the same exact integers enter one division and one log10: equal, or 1 ulp of the log10."""
import os
import re

import numpy as np
import pytest
import torch

from humannerf_amd import ops, render, scene
from humannerf_amd.config import cfg
from humannerf_amd.network import Network
from humannerf_amd.seeded import default_shapes, seeded_state, with_density

from test_metrics_cpu import cases, image_pair, make_mask

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_metrics(a, b, mask=None, data_range=1.0):
    return ops.image_metrics(T(a), T(b), T(mask), data_range).cpu().numpy()


def check(got, ref, tag):
    """(psnr, ssim) of the kernel against the twin's; returns (|d psnr| in ulp, |d ssim|)."""
    dp = 0.0
    if not (got[0] == ref[0] or (np.isnan(got[0]) and np.isnan(ref[0]))):
        dp = abs(got[0] - ref[0]) / np.spacing(abs(ref[0]))
        assert dp <= 1.0, (tag, 'psnr', got[0], ref[0])
    if np.isnan(ref[1]):
        assert np.isnan(got[1]), (tag, 'ssim', got[1])
        return dp, 0.0
    assert abs(got[1] - ref[1]) <= 1e-12, (tag, 'ssim', got[1], ref[1])
    return dp, abs(got[1] - ref[1])


@pytest.mark.parametrize('data_range', [1.0, 2.0])
def test_kernel_against_the_twin_on_the_cpu_cases(data_range):
    worst = [0.0, 0.0]
    for H, W, kind, mk in cases():
        a, b = image_pair(kind, H, W)
        mask = make_mask(mk, H, W)
        d = check(gpu_metrics(a, b, mask, data_range)[0], render.metrics_u8(a, b, mask, data_range)[0], (H, W, kind, mk))
        worst = [max(w, v) for w, v in zip(worst, d)]
    print('data_range %g: max |d psnr| %.1f ulp, max |d ssim| %.3g' % (data_range, worst[0], worst[1]))


TILING = [
    # H, W, mask box (y0, y1, x0, x1) or None
    (7, 7, None),                       # one window
    (39, 39, None),                     # one tile of 32x32 positions plus one row and one column
    (71, 71, None),                     # two tiles plus one in each direction
    (38, 45, None),                     # exactly one tile high; a width that is no multiple of 4
    (41, 70, None),
    (90, 100, (3, 60, 5, 77)),          # the box starts at odd offsets and ends inside a tile
    (90, 100, (0, 90, 0, 100)),         # the box is the whole image
    (90, 100, (51, 90, 61, 100)),       # one tile plus one, in the far corner
    (130, 300, (1, 130, 7, 299)),       # many tiles: the partials of 4 x 9 workgroups per channel
]


@pytest.mark.parametrize('H,W,box', TILING)
def test_kernel_against_the_twin_where_the_tiling_can_go_wrong(H, W, box):
    mask = None
    if box is not None:
        mask = np.zeros((H, W), np.uint8)
        mask[box[0]:box[1], box[2]:box[3]] = 7
    for kind in ('noisy', 'unrelated', 'step'):
        a, b = image_pair(kind, H, W, seed=11)
        d = check(gpu_metrics(a, b, mask)[0], render.metrics_u8(a, b, mask)[0], (H, W, box, kind))
        print(H, W, box, kind, 'd psnr %.1f ulp, d ssim %.3g' % d)


def test_a_batch_is_its_images_one_by_one_bit_for_bit():
    H, W = 70, 135
    a0, b0 = image_pair('noisy', H, W, seed=1)
    a1, b1 = image_pair('unrelated', H, W, seed=2)
    m0, m1 = make_mask('inside', H, W), make_mask('L', H, W)
    both = gpu_metrics(np.stack([a0, a1]), np.stack([b0, b1]), np.stack([m0, m1]))
    one0, one1 = gpu_metrics(a0, b0, m0), gpu_metrics(a1, b1, m1)
    assert both.shape == (2, 2)
    assert both[0].tobytes() == one0[0].tobytes() and both[1].tobytes() == one1[0].tobytes()
    check(both[0], render.metrics_u8(a0, b0, m0)[0], 'batch 0')
    check(both[1], render.metrics_u8(a1, b1, m1)[0], 'batch 1')
    # bool masks and (N, H, W, 1) masks are the same masks
    again = ops.image_metrics(T(np.stack([a0, a1])), T(np.stack([b0, b1])), T(np.stack([m0, m1]) != 0)[..., None])
    assert again.cpu().numpy().tobytes() == both.tobytes()


def test_two_calls_give_the_same_bits():
    a, b = image_pair('noisy', 130, 300, seed=4)
    pa, pb = T(a), T(b)
    first = ops.image_metrics(pa, pb).cpu().numpy()
    other = gpu_metrics(*image_pair('unrelated', 130, 300))                 # the workspace is used in between
    second = ops.image_metrics(pa, pb).cpu().numpy()
    assert first.tobytes() == second.tobytes() and first.tobytes() != other.tobytes()


def test_empty_mask_and_narrow_crop_give_nan_without_an_error():
    a, b = image_pair('noisy', 20, 20)
    m = np.zeros((20, 20), np.uint8)
    out = gpu_metrics(a, b, m)[0]
    assert np.isnan(out[0]) and np.isnan(out[1])
    m[2:12, 4:10] = 1                                                       # 6 wide
    out = gpu_metrics(a, b, m)[0]
    check(out, render.metrics_u8(a, b, m)[0], 'narrow')
    assert np.isfinite(out[0]) and np.isnan(out[1])
    small = gpu_metrics(*image_pair('noisy', 6, 30))[0]                     # an image lower than the window
    assert np.isfinite(small[0]) and np.isnan(small[1])
    same = gpu_metrics(a, a)[0]
    assert same[0] == np.inf and same[1] == 1.0


def test_sums_at_their_maximum():
    """All-255 against all-0 at 70 x 135: SSE = 255^2 * count exactly, so the PSNR is exactly 0 dB; every window sum
    is at its int32 maximum.  Every window has the same value, both sides add copies of one number: within the bound
    of the comparison above (printed: whether the bits are equal)."""
    a, b = image_pair('extremes', 70, 135)
    got, ref = gpu_metrics(a, b)[0], render.metrics_u8(a, b)[0]
    print('extremes: ssim kernel %r twin %r, same bits: %s' % (got[1], ref[1], got[1] == ref[1]))
    assert got[0] == 0.0 and ref[0] == 0.0
    assert abs(got[1] - ref[1]) <= 1e-12
    got2, ref2 = gpu_metrics(b, a, data_range=2.0)[0], render.metrics_u8(b, a, data_range=2.0)[0]
    assert got2[0] == 0.0 and abs(got2[1] - ref2[1]) <= 1e-12


def test_refusals():
    a, b = image_pair('noisy', 20, 20)
    from humannerf_amd._lib import HnrfError
    with pytest.raises(HnrfError):
        ops.image_metrics(torch.from_numpy(a), torch.from_numpy(b))                    # on the host
    with pytest.raises(HnrfError):
        ops.image_metrics(T(a).float(), T(b).float())                                  # float images
    with pytest.raises(HnrfError):
        ops.image_metrics(T(a), T(b)[:19])
    with pytest.raises(HnrfError):
        ops.image_metrics(T(a), T(b), data_range=0.0)


def test_the_op_does_not_synchronise():
    """An event recorded behind ~0.2 s of queued matrix products is still pending when ops.image_metrics returns.  The
    assertion is skipped for a try whose event happened to be complete; printed: how often."""
    a, b = image_pair('noisy', 130, 300)
    pa, pb, pm = T(a), T(b), T(make_mask('inside', 130, 300))
    x = torch.randn(8192, 8192, device=DEV)
    ops.image_metrics(pa, pb, pm)                                          # warm: workspace, code objects
    torch.mm(x, x)
    torch.cuda.synchronize()
    pending = 0
    for _ in range(3):
        for _ in range(20):
            torch.mm(x, x)
        ev = torch.cuda.Event()
        ev.record()
        out = ops.image_metrics(pa, pb, pm)
        if not ev.query():
            pending += 1
        torch.cuda.synchronize()
        check(out.cpu().numpy()[0], render.metrics_u8(a, b, make_mask('inside', 130, 300))[0], 'behind a full queue')
    print('event still pending when the op returned: %d of 3 tries' % pending)
    if pending == 0:
        pytest.skip('the queued work finished before the op returned in all 3 tries: nothing to assert')


# ------------------------------------------------------------------------------------------------------- the loops
@pytest.fixture(scope='module')
def net():
    n = Network()
    n.load_state_dict({k: torch.from_numpy(v) for k, v in with_density(seeded_state(default_shapes(), seed=0), bias_delta=5.0).items()})
    return n.to(DEV).eval()


@pytest.fixture()
def loop_cfg():
    old = (cfg.get('show_truth', False), cfg.get('show_alpha', False), cfg.amd.diagnostics, cfg.N_samples,
           cfg.amd.get('metrics', 'host'))
    cfg.amd.diagnostics, cfg.N_samples = False, 64
    yield
    cfg.show_truth, cfg.show_alpha, cfg.amd.diagnostics, cfg.N_samples, cfg.amd.metrics = old


def test_render_frames_delivers_the_metrics_behind_the_images(net, tmp_path, loop_cfg):
    from humannerf_amd import dataset
    scene.write_synthetic_subject(str(tmp_path / 'subject'), n_frames=3, size=64)
    subject = dataset.Subject(str(tmp_path / 'subject'))
    frames = [subject.movement_frame(i, load_image=True, device=DEV) for i in range(3)]
    events, images, values = [], {}, {}

    def on_image(i, rgb8, alpha8, truth8=None):
        events.append(('image', i))
        images[i] = (rgb8, alpha8, truth8)

    def on_metrics(i, v):
        events.append(('metrics', i))
        values[i] = v

    out = render.render_frames(net, frames, device=DEV, on_image=on_image, show_truth=True, metrics=['ssim', 'psnr'],
                               on_metrics=on_metrics)
    assert events == [(k, i) for i in range(3) for k in ('image', 'metrics')]
    for i in range(3):
        rgb8, _, truth8 = images[i]
        assert list(values[i]) == ['ssim', 'psnr'] and all(isinstance(v, float) for v in values[i].values())
        ref = render.metrics_u8(rgb8, truth8)[0]
        d = check(np.array([values[i]['psnr'], values[i]['ssim']]), ref, 'frame %d' % i)
        print('frame %d: psnr %.4f ssim %.6f (d %.1f ulp, %.3g)' % (i, ref[0], ref[1], d[0], d[1]))
        assert np.isfinite(ref).all()
    plain = {}
    out2 = render.render_frames(net, frames, device=DEV, on_image=lambda i, *im: plain.__setitem__(i, im), show_truth=True)
    for i in range(3):
        assert out[i].tobytes() == out2[i].tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(images[i], plain[i]))
    with pytest.raises(ValueError):
        render.render_frames(net, frames, device=DEV, metrics=['mse'])
    with pytest.raises(ValueError):
        render.render_frames(net, frames, device=DEV, metrics=['lpips'])


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def _movement(net, subject, logdir, route, metrics, lpips_fn=None):
    from humannerf_amd import run
    cfg.amd.metrics = route
    res = run.run_movement(net, subject, logdir=logdir, metrics=metrics, lpips_fn=lpips_fn)
    base = res['image_dir'].rstrip('/')
    pngs = {f: _read(os.path.join(base, f)) for f in sorted(os.listdir(base)) if f.endswith('.png')}
    with open(base + '-metrics.perimg.txt') as f:
        perimg = f.read().splitlines()
    with open(base + '-metrics.average.txt') as f:
        average = f.read().splitlines()
    return res, pngs, perimg, average


def _keep_per_image_values(monkeypatch):
    """-> list that gets every finalised MetricsWriter's name2metrics."""
    kept = []
    real = render.MetricsWriter.finalize

    def finalize(self):
        kept.append(dict(self.name2metrics))
        return real(self)

    monkeypatch.setattr(render.MetricsWriter, 'finalize', finalize)
    return kept


def test_run_movement_device_route_against_the_host_route(net, tmp_path, loop_cfg, monkeypatch):
    """Same frame names, same PNG bytes, the files in the reference's format, and the unrounded per-image values of the
    two routes (MetricsWriter.name2metrics): PSNR within 1e-4 dB, SSIM within 1e-8 (tests/test_metrics_cpu.py: the twin
    against the writer route)."""
    from humannerf_amd import dataset
    names = scene.write_synthetic_subject(str(tmp_path / 'subject'), n_frames=3, size=64)
    subject = dataset.Subject(str(tmp_path / 'subject'))
    kept = _keep_per_image_values(monkeypatch)
    host, h_png, h_per, h_avg = _movement(net, subject, str(tmp_path / 'host'), 'host', ['psnr', 'ssim'])
    devr, d_png, d_per, d_avg = _movement(net, subject, str(tmp_path / 'device'), 'device', ['psnr', 'ssim'])
    assert list(h_png) == list(d_png) == sorted(n + '.png' for n in names)
    assert h_png == d_png                                                   # same PNG bytes
    assert os.path.basename(host['image_dir'].rstrip('/')) == os.path.basename(devr['image_dir'].rstrip('/'))
    line = re.compile(r'^([^:]+): psnr-\d+\.\d{4} ssim-\d\.\d{4} $')
    assert h_per[0] == d_per[0] and h_per[0].startswith('=========') and len(d_per) == 4 == len(h_per)
    for text in (h_per, d_per):
        assert sorted(line.match(l).group(1) for l in text[1:]) == sorted(names), text
    assert len(d_avg) == 3 and re.match(r'^p:\d+\.\d{4}$', d_avg[1]) and re.match(r'^s:\d\.\d{4}$', d_avg[2]), d_avg
    h, d = kept
    assert sorted(h) == sorted(d) == sorted(names)
    for n in h:
        print(n, 'host', h[n], 'device', d[n])
        assert abs(h[n]['psnr'] - d[n]['psnr']) <= 1e-4 and abs(h[n]['ssim'] - d[n]['ssim']) <= 1e-8, (n, h[n], d[n])
    assert abs(host['metrics']['psnr'] - devr['metrics']['psnr']) <= 1e-4
    assert abs(host['metrics']['ssim'] - devr['metrics']['ssim']) <= 1e-8


def test_run_movement_device_lpips_equals_the_host_route(net, tmp_path, loop_cfg, monkeypatch):
    """metrics = ['psnr', 'lpips'] with a seeded trunk: both routes feed the same float32 k / 255 pixels to the same
    deterministic kernels; within 1e-6 relative (printed: whether the bits are equal)."""
    from humannerf_amd import dataset
    from humannerf_amd.lpips import LpipsVGG
    lp = LpipsVGG.seeded(0)
    scene.write_synthetic_subject(str(tmp_path / 'subject'), n_frames=3, size=64)
    subject = dataset.Subject(str(tmp_path / 'subject'))
    kept = _keep_per_image_values(monkeypatch)
    _, h_png, h_per, _ = _movement(net, subject, str(tmp_path / 'host'), 'host', ['psnr', 'lpips'], lp.metric)
    _, d_png, d_per, _ = _movement(net, subject, str(tmp_path / 'device'), 'device', ['psnr', 'lpips'], lp.metric)
    assert h_png == d_png
    h, d = kept
    for n in h:
        print(n, 'lpips x 1000 host %r device %r same bits: %s' % (h[n]['lpips'], d[n]['lpips'], h[n]['lpips'] == d[n]['lpips']))
        assert h[n]['lpips'] > 0 and abs(h[n]['lpips'] - d[n]['lpips']) <= 1e-6 * abs(h[n]['lpips'])
        assert abs(h[n]['psnr'] - d[n]['psnr']) <= 1e-4
    assert all(re.match(r'^[^:]+: psnr-\d+\.\d{4} lpips-\d+\.\d{4} $', l) for l in d_per[1:]), d_per
