"""Image metrics on 8-bit images without a GPU: render.metrics_u8 (the numpy twin of hnrf_image_metrics) against
render.ssim / an fp64 PSNR and against the route MetricsWriter.append takes today, the argument checks of the C entry
point, MetricsWriter.append_values and the cfg.amd.metrics option.  ``cases()`` is shared with tests/test_gpu_metrics.py.
"""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from humannerf_amd import render
from humannerf_amd.config import check_amd_options, get_cfg_defaults

SIZES = [(7, 7), (8, 9), (33, 70), (70, 135)]
KINDS = ['noisy', 'step', 'unrelated', 'extremes', 'identical']
MASKS = ['none', 'inside', 'two_borders', 'seven_wide', 'L']


def image_pair(kind, H, W, seed=0):
    rs = np.random.RandomState(seed + 1000 * H + W)
    if kind == 'noisy':                                   # a picture and a noisy copy of it
        a = rs.randint(0, 256, (H, W, 3))
        b = np.clip(a + rs.randint(-12, 13, (H, W, 3)), 0, 255)
    elif kind == 'step':                                  # flat, one grey level up in the right half of one image
        a = np.full((H, W, 3), 100)
        b = a.copy()
        b[:, W // 2:] += 1
    elif kind == 'unrelated':
        a, b = rs.randint(0, 256, (H, W, 3)), rs.randint(0, 256, (H, W, 3))
    elif kind == 'extremes':                              # every sum at its maximum
        a, b = np.full((H, W, 3), 255), np.zeros((H, W, 3))
    else:
        a = rs.randint(0, 256, (H, W, 3))
        b = a.copy()
    return a.astype(np.uint8), b.astype(np.uint8)


def make_mask(kind, H, W):
    """uint8 (H, W) or None.  On the two smallest sizes some crops are narrower than the window: both sides then say NaN."""
    if kind == 'none':
        return None
    m = np.zeros((H, W), np.uint8)
    if kind == 'inside':                                  # strictly inside, odd offsets
        m[1:H - 2, 3:W - 1] = 1
    elif kind == 'two_borders':                           # touches the bottom and the right border
        m[H // 3:, W // 4:] = 255
    elif kind == 'seven_wide':                            # exactly one window wide
        m[0:H, min(5, W - 7):min(5, W - 7) + 7] = 1
    else:                                                 # L: the bounding box is larger than the support
        m[1:H - 1, 1:3] = 1
        m[H - 3:H - 1, 1:W - 1] = 1
    return m


def cases():
    for H, W in SIZES:
        for kind in KINDS:
            for mk in MASKS:
                yield H, W, kind, mk


def host_ssim(a, b, mask, data_range):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                   # the narrow crop: mean of an empty slice
        return render.ssim(a / 255.0, b / 255.0, mask, data_range)


def psnr64(a, b, mask):
    d = (a / 255.0 - b / 255.0) ** 2
    if mask is not None:
        d = d[mask != 0]
    with np.errstate(divide='ignore'):
        return -10.0 * np.log10(d.mean(dtype=np.float64))


def close(x, y, tol):
    """Within ``tol``; infinities (equal pixels under the mask) must agree exactly."""
    return x == y or abs(x - y) <= tol


@pytest.mark.parametrize('data_range', [1.0, 2.0])
def test_twin_against_render_ssim_and_fp64_psnr(data_range):
    """Both sides are fp64 statements of one expression; they differ by scipy's running-sum rounding amplified by at
    most 1 / C2.  SSIM within 1e-10, PSNR within 1e-9 dB, identical pairs: |SSIM - 1| <= 1e-12 and PSNR inf."""
    worst_s = worst_p = 0.0
    n_nan = 0
    for H, W, kind, mk in cases():
        a, b = image_pair(kind, H, W)
        mask = make_mask(mk, H, W)
        psnr, ssim = render.metrics_u8(a, b, mask, data_range)[0]
        ref_s, ref_p = host_ssim(a, b, mask, data_range), psnr64(a, b, mask)
        tag = (H, W, kind, mk)
        if np.isnan(ref_s):
            n_nan += 1
            assert np.isnan(ssim), tag
        else:
            assert abs(ssim - ref_s) <= 1e-10, (tag, ssim, ref_s)
            worst_s = max(worst_s, abs(ssim - ref_s))
        if kind == 'identical':
            assert psnr == np.inf and ref_p == np.inf, tag
            assert np.isnan(ssim) or abs(ssim - 1.0) <= 1e-12, (tag, ssim)
        else:
            assert close(psnr, ref_p, 1e-9), (tag, psnr, ref_p)
            worst_p = max(worst_p, 0.0 if psnr == ref_p else abs(psnr - ref_p))
        if kind == 'extremes':
            assert psnr == 0.0, tag
    print('data_range %g: max |d ssim| %.3g, max |d psnr| %.3g dB, %d narrow crops' % (data_range, worst_s, worst_p, n_nan))
    assert n_nan < sum(1 for _ in cases()) // 3           # (the NaN cases are the small sizes' masks only)


def test_twin_nan_cases_and_batches():
    a, b = image_pair('noisy', 20, 20)
    m = np.zeros((20, 20), np.uint8)
    m[2:12, 4:10] = 1                                     # crop 6 wide
    out = render.metrics_u8(a, b, m)[0]
    assert np.isfinite(out[0]) and np.isnan(out[1])
    m[:] = 0
    m[7, 9] = 1                                           # single pixel
    out = render.metrics_u8(a, b, m)[0]
    assert np.isfinite(out[0]) and np.isnan(out[1])
    assert np.isnan(render.metrics_u8(a, b, np.zeros((20, 20), np.uint8))).all()      # empty mask
    # a batch is its images one by one; (H, W, 1) masks are taken
    a2, b2 = image_pair('unrelated', 20, 20, seed=3)
    m2 = make_mask('L', 20, 20)
    m1 = make_mask('inside', 20, 20)
    both = render.metrics_u8(np.stack([a, a2]), np.stack([b, b2]), np.stack([m1, m2])[..., None])
    assert both.shape == (2, 2) and both.dtype == np.float64
    assert np.array_equal(both[0], render.metrics_u8(a, b, m1)[0]) and np.array_equal(both[1], render.metrics_u8(a2, b2, m2)[0])
    with pytest.raises(ValueError):
        render.metrics_u8(a.astype(np.float32), b.astype(np.float32))


def test_twin_against_the_writer_route():
    """MetricsWriter.append today: float32 k / 255 tensors through render.psnr (a float32 pairwise mean of <= 1e6
    terms: ~1.5e-6 relative = 7e-6 dB; bound 1e-4 dB) and render.ssim (float32-rounded pixels; bound 1e-8)."""
    worst_s = worst_p = 0.0
    for H, W, kind, mk in cases():
        a, b = image_pair(kind, H, W)
        mask = make_mask(mk, H, W)
        psnr, ssim = render.metrics_u8(a, b, mask)[0]
        p, t = render.MetricsWriter.normalize(a), render.MetricsWriter.normalize(b)
        assert p.dtype == torch.float32
        tm = None if mask is None else torch.from_numpy(mask != 0)[..., None]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ws = render.ssim(p, t, mask)
        wp = render.psnr(p, t, tm).item()
        if np.isnan(ws):
            assert np.isnan(ssim)
        else:
            assert abs(ssim - ws) <= 1e-8, ((H, W, kind, mk), ssim, ws)
            worst_s = max(worst_s, abs(ssim - ws))
        if kind == 'identical':
            assert psnr == np.inf and wp == np.inf
        else:
            assert close(psnr, wp, 1e-4), ((H, W, kind, mk), psnr, wp)
            worst_p = max(worst_p, 0.0 if psnr == wp else abs(psnr - wp))
    print('writer route: max |d ssim| %.3g, max |d psnr| %.3g dB' % (worst_s, worst_p))


def test_image_metrics_argument_errors_do_not_need_a_gpu():
    from humannerf_amd import _lib
    lib = _lib.load()
    err = lambda: lib.hnrf_last_error().decode()
    assert lib.hnrf_image_metrics(None, None, None, 1, 8, 8, 1.0, None, 0, None, None) == -1 and 'null pointer' in err()
    assert lib.hnrf_image_metrics(256, 256, None, 1, 8, 8, 1.0, 256, 1 << 20, None, None) == -1 and 'null pointer' in err()
    assert lib.hnrf_image_metrics(256, 256, None, 1, 0, 8, 1.0, 256, 1 << 20, 256, None) == -2 and '0x8' in err()
    assert lib.hnrf_image_metrics(256, 256, None, 0, 8, 8, 1.0, 256, 1 << 20, 256, None) == -2
    assert lib.hnrf_image_metrics(256, 256, None, 1, 8, 9000, 1.0, 256, 1 << 20, 256, None) == -2
    assert lib.hnrf_image_metrics(256, 256, None, 1, 8, 8, 0.0, 256, 1 << 20, 256, None) == -2 and 'data_range' in err()
    need = lib.hnrf_image_metrics_workspace_bytes(2, 70, 135)
    assert need > 0 and need % 256 == 0
    assert lib.hnrf_image_metrics(256, 256, None, 2, 70, 135, 1.0, 256, need - 1, 256, None) == -4 and 'workspace' in err()
    assert lib.hnrf_image_metrics_workspace_bytes(1, 0, 8) == 0 and lib.hnrf_image_metrics_workspace_bytes(0, 8, 8) == 0
    assert lib.hnrf_abi_version() == 13
    assert _lib.SIGNATURES['hnrf_image_metrics'][1][6] is ctypes.c_double


def test_append_values_writes_what_append_writes(tmp_path):
    a, b = image_pair('noisy', 33, 70)
    a2, b2 = image_pair('noisy', 33, 70, seed=5)
    one = render.MetricsWriter(str(tmp_path / 'a'), 'movement', dataset='d', metrics=['psnr', 'ssim'])
    two = render.MetricsWriter(str(tmp_path / 'b'), 'movement', dataset='d', metrics=['psnr', 'ssim'])
    for name, (p, t) in (('frame_000000', (a, b)), ('frame_000001', (a2, b2))):
        one.append(name, p, t)
        two.append_values(name, dict(one.name2metrics[name]))
    with pytest.raises(AssertionError):
        two.append_values('frame_000001', {'psnr': 1.0, 'ssim': 1.0})
    two.N -= 1                                            # (the refused line counted)
    avg1, avg2 = one.finalize(), two.finalize()
    assert avg1 == avg2 and two.name2metrics == one.name2metrics
    for f in ('movement-metrics.perimg.txt', 'movement-metrics.average.txt'):
        with open(tmp_path / 'a' / f) as fa, open(tmp_path / 'b' / f) as fb:
            ta, tb = fa.read(), fb.read()
        assert ta == tb and len(ta.splitlines()) == 3
    with open(tmp_path / 'b' / 'movement-metrics.perimg.txt') as f:
        lines = f.read().splitlines()[1:]
    assert all(re.match(r'^frame_\d{6}: psnr-\d+\.\d{4} ssim-\d\.\d{4} $', l) for l in lines), lines


def test_the_metrics_option_is_validated():
    c = get_cfg_defaults()
    assert c.amd.metrics == 'host'
    check_amd_options(c.amd)
    c.amd.metrics = 'device'
    assert check_amd_options(c.amd) == ('mlp', 'mlp', 128)
    c.amd.metrics = 'gpu'
    with pytest.raises(ValueError, match='metrics'):
        check_amd_options(c.amd)


def test_device_metrics_refuse_a_cpu_device():
    from humannerf_amd import run
    from humannerf_amd.config import cfg
    old = cfg.amd.get('metrics', 'host')
    cfg.amd.metrics = 'device'
    try:
        with pytest.raises(ValueError, match='needs a GPU'):
            run.run_movement(None, None, device=torch.device('cpu'), metrics=['psnr', 'ssim'])
    finally:
        cfg.amd.metrics = old
    with pytest.raises(ValueError, match='need a GPU'):
        render.render_frames(torch.nn.Linear(1, 1), [], device=torch.device('cpu'), metrics=['psnr'])
