"""The seeded test images of the JPEG encoder (tests/test_video_cpu.py, tests/test_gpu_video.py) and what each is there
for.  Built once per process; the twin's streams and counters are computed once and shared."""
import functools
import io

import numpy as np

QUALITIES = (10, 50, 90, 100)

# Decoded PSNR against the source may fall below PIL's own encode of the same image at the same quality by this much
# (dB), q in {10, 50, 90}.  Provenance: the largest shortfall of the twin over the images below, measured with PIL's
# libjpeg on the CPU, is 0.159 dB (40x24, q = 10); doubled.  Several tenths of a dB would mean a wrong transform.
PSNR_MARGIN_DB = 0.32


@functools.lru_cache(maxsize=None)
def images():
    """name -> (H, W, 3) uint8, read-only."""
    rs = np.random.RandomState(0)
    out = {}
    out['1x1'] = rs.randint(0, 256, (1, 1, 3)).astype(np.uint8)                                     # all padding
    y, x = np.mgrid[0:16, 0:16]
    out['16x16_smooth'] = np.stack([128 + 100 * np.sin(x / 5), 128 + 100 * np.cos(y / 7), 8 * x + 4 * y],
                                   -1).clip(0, 255).astype(np.uint8)                                # one MCU, no RST
    y, x = np.mgrid[0:24, 0:40]
    out['40x24'] = np.stack([128 + 100 * np.sin(x / 5 + y / 9), 128 + 100 * np.cos(y / 7), 5 * x + 2 * y],
                            -1).clip(0, 255).astype(np.uint8)                                       # padding in both axes
    out['17x33_bw'] = (rs.rand(33, 17, 1) > .5).astype(np.uint8).repeat(3, 2) * 255                 # odd sizes, binary
    y, x = np.mgrid[0:48, 0:144]
    a = np.stack([128 + 120 * np.sin(x / 9 + y / 5), 128 + 120 * np.cos(y / 6 - x / 11), 128 + 120 * np.sin(x / 4)],
                 -1).clip(0, 255).astype(np.uint8)
    a[8:40, 30:90] = (255, 0, 0)
    out['144x48_rect'] = a                                               # 27 MCUs: RST wraps three times; DC category 11
    out['48x48_noise'] = rs.randint(0, 256, (48, 48, 3)).astype(np.uint8)
    out['48x48_sparse'] = ((rs.rand(48, 48, 1) < .02) * 255).astype(np.uint8).repeat(3, 2)
    # 1056 MCUs: more than the 256 the scan's block takes per pass (five passes, the last one partial)
    out['528x512_noise'] = rs.randint(0, 256, (512, 528, 3)).astype(np.uint8)
    for v in out.values():
        v.setflags(write=False)
    return out


CASES = [(name, q) for name in ('1x1', '16x16_smooth', '40x24', '17x33_bw', '144x48_rect', '48x48_noise', '48x48_sparse',
                                '528x512_noise') for q in QUALITIES]


@functools.lru_cache(maxsize=None)
def twin(name, q):
    """(stream bytes, counters) of the numpy twin."""
    from humannerf_amd import video
    counters = {}
    return video.jpeg_encode_numpy(images()[name], q, counters), counters


def decode(stream):
    """(decoded RGB uint8 array, PIL's quantization dict); warnings are errors."""
    import warnings
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        im = Image.open(io.BytesIO(stream))
        im.load()
        return np.asarray(im.convert('RGB')), {k: list(v) for k, v in im.quantization.items()}


@functools.lru_cache(maxsize=None)
def pil_encode(name, q):
    return pil_encode_array(images()[name], q)


def pil_encode_array(a, q):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a)).save(b, 'JPEG', quality=q, subsampling=2)
    return b.getvalue()


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = (d * d).mean()
    return float('inf') if mse == 0 else 10 * np.log10(65025.0 / mse)
