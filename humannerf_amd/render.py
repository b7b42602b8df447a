"""Frame-sharded rendering driver and the image side of the path ("next" row).

What run.py does per frame (run.py:68-157, 214-445): ``model(**data, iter_val=cfg.eval_iter)`` under no_grad, scatter
the rendered rays back into the H x W image by ``ray_mask`` with background fill (run.py:48-65), quantise to 8 bit,
write PNGs / a video, append metrics.  Here the scatter / quantisation runs on the GPU, frames are dealt round-robin
over the ranks (one process per GPU, no data-path collective), what a finished frame sends to the host (uint8 images,
metric vector, JPEG stream) travels asynchronously through pinned buffers and PNG encoding happens on worker threads,
so that the GPU never waits for an image to be written.  That copy-out is stated once, FrameOutbox, for every loop that
renders frames: render_frames here, run.run_mesh_render.

  unpack_to_image, to_8b_image, to_8b3ch_image, tile_images   run.py:37-65, image_util.py:21-53   (byte-exact:
                                                              tests/golden/image_unpack.npz, made by the reference)
  psnr, MetricsWriter                                         metrics_util.py:9-88                (same fixture)
  ssim                                                        metrics_util.py:90-106 calls skimage -- not importable
                                                              here: the published algorithm, parity unpinned
  metrics_u8                                                  psnr / ssim of 8-bit images from exact integer moments: the
                                                              numpy twin of ops.image_metrics (csrc/hnrf_metrics.hip), which
                                                              render_frames(metrics=...) runs on the device
  ImageWriter                                                 image_util.py:55-128 (PNG via PIL; the MP4 of finalize()
                                                              needs imageio, which is absent: frames + .npy instead;
                                                              a Motion-JPEG .avi: render_frames(video=...), video.py)
"""
import os
import queue
import threading
import time
from collections import defaultdict, namedtuple

import numpy as np
import torch

from . import dist as hdist
from .config import cfg, quiet_gc


# --------------------------------------------------------------------------------------------- image helpers
def to_8b_image(image):
    """(255 * clip(image, 0, 1)) truncated to uint8 (image_util.py:21-22); numpy array or tensor."""
    if torch.is_tensor(image):
        return (255.0 * image.clamp(0.0, 1.0)).to(torch.uint8)
    return (255. * np.clip(image, 0., 1.)).astype(np.uint8)


def to_3ch_image(image):
    """(H, W) or (H, W, 1) -> (H, W, 3) (image_util.py:25-33)."""
    if torch.is_tensor(image):
        if image.dim() == 2:
            return torch.stack([image, image, image], dim=-1)
        assert image.dim() == 3 and image.shape[2] == 1
        return torch.cat([image, image, image], dim=-1)
    if image.ndim == 2:
        return np.stack([image, image, image], axis=-1)
    assert image.ndim == 3 and image.shape[2] == 1
    return np.concatenate([image, image, image], axis=-1)


def to_8b3ch_image(image):
    return to_3ch_image(to_8b_image(image))


def tile_images(images, imgs_per_row=4):
    """Mosaic of equally sized images, rows of ``imgs_per_row``; an incomplete last row is dropped, and so is a
    last row that differs from the one before once there are more than two (image_util.py:40-53)."""
    rows, row = [], []
    imgs_per_row = min(len(images), imgs_per_row)
    for img in images:
        row.append(img)
        if len(row) == imgs_per_row:
            rows.append(np.concatenate(row, axis=1))
            row = []
    if len(rows) > 2 and len(rows[-1]) != len(rows[-2]):
        rows.pop()
    return np.concatenate(rows, axis=0)


def unpack_to_image(width, height, ray_mask, bgcolor, rgb, alpha, truth=None, ray_index=None):
    """Device-side restatement of run.py:48-65.  ``bgcolor`` in 0..1 like the reference's call sites pass it
    (run.py:127-131); ``rgb`` (N, 3), ``alpha`` (N,), optional ``truth`` (N, 3) for the rays selected by ``ray_mask``
    (H*W,) bool.  Returns (rgb uint8 (H,W,3), alpha uint8 (H,W,3), truth uint8 (H,W,3)); without ``truth`` the third
    entry is the float32 (H*W, 3) background plane, as in the reference.
    ``ray_index`` (N,) int64 = the positions where ``ray_mask`` is set: with it the scatter is an index_copy and nothing
    here waits for the device (a boolean-mask assignment counts the set bits on the host: one synchronisation per
    image, which is what kept the frame loop from running ahead of the GPU)."""
    dev = rgb.device
    bg = torch.as_tensor(bgcolor, dtype=torch.float32, device=dev).reshape(1, 3)
    if ray_index is None:
        ray_index = torch.nonzero(torch.as_tensor(ray_mask, device=dev).reshape(-1)).reshape(-1)
    img = bg.repeat(height * width, 1)
    img.index_copy_(0, ray_index, rgb.to(torch.float32))
    rgb8 = to_8b_image(img).reshape(height, width, 3)
    truth_img = bg.repeat(height * width, 1)
    if truth is not None:
        truth_img.index_copy_(0, ray_index, torch.as_tensor(truth, dtype=torch.float32, device=dev))
        truth_img = to_8b_image(truth_img).reshape(height, width, 3)
    amap = torch.zeros(height * width, dtype=torch.float32, device=dev)
    amap.index_copy_(0, ray_index, alpha.to(torch.float32))
    a8 = to_8b3ch_image(amap.reshape(height, width)).contiguous()
    return rgb8, a8, truth_img


# --------------------------------------------------------------------------------------------- metrics
def psnr(pred, target, mask=None):
    """-10 log10(mse), maximum pixel value 1; optional (H, W, 1) bool mask tiled over the channels
    (metrics_util.py:75-88)."""
    if mask is not None:
        mask = torch.tile(torch.as_tensor(mask), [1, 1, 3])
        pred, target = pred[mask], target[mask]
    mse = ((pred - target) ** 2).mean()
    return -10.0 * torch.log(mse) / np.log(10.0)


def ssim(pred, target, mask=None, data_range=1.0):
    """Mean structural similarity (Wang et al. 2004) with the defaults skimage.metrics.structural_similarity uses for
    float images: 7x7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance, per-channel mean, borders cropped
    by half a window; with ``mask`` the images are cropped to the mask's bounding box first (metrics_util.py:90-106).
    PARITY UNPINNED: skimage is not importable in the build container, so no reference-generated vector exists."""
    from scipy.ndimage import uniform_filter
    a = np.asarray(pred.cpu() if torch.is_tensor(pred) else pred, dtype=np.float64)
    b = np.asarray(target.cpu() if torch.is_tensor(target) else target, dtype=np.float64)
    assert a.shape == b.shape
    if mask is not None:
        m = np.asarray(mask.cpu() if torch.is_tensor(mask) else mask).reshape(a.shape[0], a.shape[1]) != 0
        ys, xs = np.where(m)
        a, b = a[ys.min():ys.max() + 1, xs.min():xs.max() + 1], b[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
    win, k1, k2 = 7, 0.01, 0.03
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    cov_norm = win * win / (win * win - 1.0)
    vals = []
    for ch in range(a.shape[2] if a.ndim == 3 else 1):
        x, y = (a[..., ch], b[..., ch]) if a.ndim == 3 else (a, b)
        ux, uy = uniform_filter(x, win), uniform_filter(y, win)
        uxx, uyy, uxy = uniform_filter(x * x, win), uniform_filter(y * y, win), uniform_filter(x * y, win)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        pad = (win - 1) // 2
        vals.append(s[pad:s.shape[0] - pad, pad:s.shape[1] - pad].mean())
    return float(np.mean(vals))


def metrics_u8(pred, target, mask=None, data_range=1.0):
    """PSNR and SSIM of uint8 images, (H, W, 3) or (N, H, W, 3), as ``psnr`` / ``ssim`` above define them for the pixels
    k / 255 -- the numpy twin of the device kernel (ops.image_metrics, csrc/hnrf_metrics.hip) and the CPU statement
    its tests compare against.  ``mask``: (H, W[, 1]) or (N, H, W[, 1]), non-zero = inside.  Returns float64 (n, 2):
    psnr, ssim per image.

    The inputs are 8-bit, so everything up to the closed form is exact integer arithmetic: SSE is an integer sum,
    psnr = -10 log10(SSE / (255^2 count)), count = 3 H W or 3 nnz(mask); the window moments are integer 7x7 sums Sx, Sy,
    Sxx, Syy, Sxy, with ux = Sx / (49 * 255), uxx = Sxx / (49 * 255^2) (one rounding each) entering ``ssim``'s fp64
    expression in its operand order.  A window's value has the same bits here and in the kernel; only the order of the
    sum over the windows differs (numpy adds pairwise).  Equal images give psnr +inf; an empty mask gives (NaN, NaN)
    and a crop narrower than the window gives ssim NaN (``ssim`` returns NaN for the narrow crop and raises for the
    empty mask)."""
    a, b = np.asarray(pred), np.asarray(target)
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.shape != b.shape or a.ndim not in (3, 4) or a.shape[-1] != 3:
        raise ValueError('metrics_u8 takes two uint8 images (H, W, 3) or (N, H, W, 3) of one shape')
    if a.ndim == 3:
        a, b = a[None], b[None]
    n, H, W, _ = a.shape
    m = None if mask is None else (np.asarray(mask).reshape(n, H, W) != 0)
    win = 7
    c1, c2 = (0.01 * data_range) * (0.01 * data_range), (0.03 * data_range) * (0.03 * data_range)
    cov_norm = win * win / (win * win - 1.0)

    def window_sums(v):                                                  # (h, w) int64 -> (h - 6, w - 6) exact 7x7 sums
        c = np.zeros((v.shape[0] + 1, v.shape[1] + 1), dtype=np.int64)
        c[1:, 1:] = v.cumsum(0).cumsum(1)
        return c[win:, win:] - c[:-win, win:] - c[win:, :-win] + c[:-win, :-win]

    out = np.empty((n, 2), dtype=np.float64)
    for i in range(n):
        x, y = a[i].astype(np.int64), b[i].astype(np.int64)
        inside = np.ones((H, W), dtype=bool) if m is None else m[i]
        sse, count = int((((x - y) ** 2).sum(-1))[inside].sum()), 3 * int(inside.sum())
        with np.errstate(divide='ignore', invalid='ignore'):
            out[i, 0] = -10.0 * np.log10(np.float64(sse) / (65025.0 * np.float64(count)))
        ys, xs = np.where(inside)
        if ys.size == 0 or ys.max() - ys.min() + 1 < win or xs.max() - xs.min() + 1 < win:
            out[i, 1] = np.nan
            continue
        x, y = x[ys.min():ys.max() + 1, xs.min():xs.max() + 1], y[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
        vals = []
        for ch in range(3):
            p, q = x[..., ch], y[..., ch]
            ux, uy = window_sums(p) / 12495.0, window_sums(q) / 12495.0
            uxx, uyy, uxy = window_sums(p * p) / 3186225.0, window_sums(q * q) / 3186225.0, window_sums(p * q) / 3186225.0
            vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
            s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
            vals.append(s.mean())
        out[i, 1] = ((vals[0] + vals[1]) + vals[2]) / 3.0
    return out


class MetricsWriter:
    """Per-image and average metric text files in the reference's format (metrics_util.py:9-60): ``<exp>-metrics.
    perimg.txt`` gets ``name: psnr-26.2530 ssim-0.9123 `` per image, ``<exp>-metrics.average.txt`` gets
    ``p:26.3092`` (first letter of the metric).  ``metrics`` defaults to cfg.eval.metrics or ['psnr']; 'lpips' needs a
    caller-supplied ``lpips_fn(pred, target)`` (the VGG trunk cannot be fetched offline)."""

    def __init__(self, output_dir, exp_name, dataset, metrics=None, lpips_fn=None):
        os.makedirs(output_dir, exist_ok=True)
        self.per_img_f = open(os.path.join(output_dir, '%s-metrics.perimg.txt' % exp_name), 'a')
        self.average_f = open(os.path.join(output_dir, '%s-metrics.average.txt' % exp_name), 'a')
        self.per_img_f.writelines('=========%s==========\n' % dataset)
        self.average_f.writelines('=========%s==========\n' % dataset)
        self.metrics = list(metrics if metrics is not None else cfg.get('eval', {}).get('metrics', ['psnr']))
        if 'lpips' in self.metrics and lpips_fn is None:
            raise ValueError('metric lpips needs an lpips_fn (LPIPS-VGG weights are not obtainable offline)')
        self.funcs = {'psnr': lambda p, t, m: psnr(p, t, m).item(),
                      'ssim': lambda p, t, m: ssim(p, t, m),
                      'lpips': lambda p, t, m: 1000 * float(lpips_fn(p, t))}
        self.name2metrics, self.sums, self.N = {}, defaultdict(float), 0

    @staticmethod
    def normalize(img):
        if isinstance(img, np.ndarray):
            img = torch.tensor(img, dtype=torch.float32)
        if torch.max(img) > 2:
            img = img / 255
        return img

    def append(self, name, pred, target, mask=None):
        self.N += 1
        assert name not in self.name2metrics, name
        pred, target = self.normalize(pred), self.normalize(target)
        self.per_img_f.writelines('%s: ' % name)
        self.name2metrics[name] = {}
        for k in self.metrics:
            v = self.funcs[k](pred, target, mask)
            self.name2metrics[name][k] = v
            self.sums[k] += v
            self.per_img_f.writelines('{}-{:.4f} '.format(k, v))
        self.per_img_f.writelines('\n')

    def append_values(self, name, values):
        """The bookkeeping and the line of ``append`` for metric values computed elsewhere (``values``: {metric: float}
        holding every entry of ``self.metrics``; render_frames(on_metrics=...) with cfg.amd.metrics = 'device')."""
        self.N += 1
        assert name not in self.name2metrics, name
        self.per_img_f.writelines('%s: ' % name)
        self.name2metrics[name] = {}
        for k in self.metrics:
            v = float(values[k])
            self.name2metrics[name][k] = v
            self.sums[k] += v
            self.per_img_f.writelines('{}-{:.4f} '.format(k, v))
        self.per_img_f.writelines('\n')

    def finalize(self):
        averages = {k: v / self.N for k, v in self.sums.items()}
        for k, v in averages.items():
            self.average_f.writelines('%s:%.4f\n' % (k[0], v))
        self.per_img_f.close()
        self.average_f.close()
        return averages


class ImageWriter:
    """PNG writer of the render drivers (image_util.py:55-128): ``<output_dir>/<exp_name>/<name or %06d>.png``.
    Encoding runs on ``workers`` threads behind a bounded queue (PIL releases the GIL while it compresses), so
    ``append`` returns at once and can be used as ``render_frames(on_image=...)``; ``finalize`` drains the queue.  The
    reference's finalize() also writes an MP4 through imageio (fps 10, quality 8): done when imageio is importable;
    it is not in this image, so the frames are then stacked into ``<exp_name>.npy`` (sorted by name like the
    reference).  A video without imageio comes from cfg.amd.video = 'mjpeg' / 'mjpeg_only': the run_* loops then
    JPEG-encode every frame's panels on the device and write ``<exp_name>.avi`` (Motion-JPEG, humannerf_amd/video.py)
    next to, or instead of, what this class writes; this class is unchanged by it.  ``append_3d`` / ``append_cnl_3d`` write the point clouds of
    run.py's 3-D dumps as Wavefront .obj text exactly like image_util.py:85-109."""

    def __init__(self, output_dir, exp_name, workers=4, keep_frames=True):
        from PIL import Image
        self._Image = Image
        self.output_dir = output_dir
        self.image_dir = os.path.join(output_dir, exp_name)
        self.obj_dir = os.path.join(output_dir, exp_name + '_3d')
        os.makedirs(self.image_dir, exist_ok=True)
        self.frame_idx = -1
        self.keep = keep_frames
        self.images_np, self.image_names = [], []
        self.name_3d_together = {}
        self._q = queue.Queue(maxsize=4 * workers)
        self._err = []
        self._threads = [threading.Thread(target=self._work, daemon=True) for _ in range(workers)]
        for t in self._threads:
            t.start()

    def _work(self):
        while True:
            item = self._q.get()
            if item is None:
                return
            try:
                self._Image.fromarray(item[0]).save(item[1])
            except Exception as e:               # surfaced by finalize()
                self._err.append(e)

    def append(self, image, img_name=None):
        self.frame_idx += 1
        if img_name is None:
            img_name = '%06d' % self.frame_idx
        image = np.ascontiguousarray(image)
        self._q.put((image, os.path.join(self.image_dir, '%s.png' % img_name)))
        if self.keep:
            self.images_np.append(image)
            self.image_names.append(img_name)
        return self.frame_idx, img_name

    def append_3d(self, point3d, mask, obj_name=None, weight_img=None, depth_img=None):
        """(H, W, 3) positions of the pixels where ``mask`` is set as 'v x y z' lines (image_util.py:85-97)."""
        os.makedirs(self.obj_dir, exist_ok=True)
        obj_name = '%06d' % self.frame_idx if obj_name is None else obj_name
        us, vs = np.nonzero(mask)
        with open(os.path.join(self.obj_dir, obj_name + '.obj'), 'w') as f:
            f.writelines('v %.7f %.7f %.7f\n' % tuple(point3d[u, v]) for u, v in zip(us, vs))
        if weight_img is not None:
            np.save(os.path.join(self.obj_dir, obj_name + '-weights.npy'), weight_img)
        if depth_img is not None:
            np.save(os.path.join(self.obj_dir, obj_name + '-depth.npy'), depth_img)

    def append_cnl_3d(self, cnl_xyz, cnl_rgb, obj_name=None):
        """Coloured canonical points: 'v x y z r g b ' lines (image_util.py:102-109)."""
        os.makedirs(self.obj_dir, exist_ok=True)
        obj_name = '%06d-cnl' % self.frame_idx if obj_name is None else obj_name
        with open(os.path.join(self.obj_dir, obj_name + '.obj'), 'w') as f:
            f.writelines('v %.7f %.7f %.7f %.7f %.7f %.7f \n' % (*xyz, *rgb) for xyz, rgb in zip(cnl_xyz, cnl_rgb))

    def append_3d_together(self, name, data):
        """One frame's [N, 10] record tensor (moved to the host here), kept until finalize."""
        self.name_3d_together[name] = torch.as_tensor(data).detach().cpu()

    def finalize(self, video_name=None):
        for _ in self._threads:
            self._q.put(None)
        for t in self._threads:
            t.join()
        if self._err:
            raise self._err[0]
        if self.name_3d_together:
            self.path_3d_together = os.path.join(self.output_dir, 'name-2-3d.bin')
            torch.save(self.name_3d_together, self.path_3d_together)
        if self.keep and self.images_np:
            order = sorted(range(len(self.images_np)), key=lambda i: self.image_names[i])
            stack = np.stack([self.images_np[i] for i in order], axis=0)
            try:
                import imageio
            except ImportError:
                imageio = None
            if imageio is not None:                                              # image_util.py:122-128
                path = (self.image_dir.rstrip('/') + '.mp4') if video_name is None else os.path.join(self.image_dir, video_name)
                imageio.mimwrite(path, stack, format='mp4', fps=10, quality=8)
                return path
            path = (self.image_dir.rstrip('/') + '.npy') if video_name is None else os.path.join(self.image_dir, video_name + '.npy')
            np.save(path, stack)
            return path
        return None


# --------------------------------------------------------------------------------------------- frame loop
class _PinnedPool:
    """A few page-locked staging buffers per shape and dtype (uint8 images; the float64 metric vector of a frame):
    device -> host copies into pageable memory are staged and synchronous inside the runtime; into pinned memory they
    are real asynchronous DMA."""

    def __init__(self):
        self.free = defaultdict(list)

    def take(self, shape, dtype=torch.uint8):
        lst = self.free[(tuple(shape), dtype)]
        return lst.pop() if lst else torch.empty(tuple(shape), dtype=dtype, pin_memory=True)

    def give(self, t):
        self.free[(tuple(t.shape), t.dtype)].append(t)


def video_copy_cap(height, width):
    """Bytes of a frame's JPEG stream that FrameOutbox.post copies to the host before it knows the stream's length:
    3 bits per pixel of the panels, at least 64 KiB.  (A 512 x 512 render panel at quality 90 takes 15-40 KB; 3 bits per
    pixel is what dense texture takes at that quality.)  A longer stream costs one synchronous copy of the remainder when
    the frame is handed over, counted in render_frames.last_video['fallbacks']."""
    return max(64 << 10, (3 * height * width) // 8)


class _Parcel:
    """One frame's host-bound products between FrameOutbox.post and the hand-over: the staged 8-bit images, the staged
    metric vector or None, the staged first ``cap`` bytes of the JPEG stream with its length word (and the device buffer
    a longer stream's remainder is fetched from) or None, all behind one ``event`` (None on a CPU device, where the
    tensors themselves stand in for the pinned copies and ``pool`` is None).  ``collect`` or ``discard`` ends it: once."""

    def __init__(self, pool, event, hosts, metric_host, vhost, lhost, vdev, cap, map_hosts=None):
        self.pool, self.event, self.hosts, self.metric_host = pool, event, hosts, metric_host
        self.vhost, self.lhost, self.vdev, self.cap = vhost, lhost, vdev, cap
        # the staged geometry panels {name: buffer} (render_frames(maps=...)) or None; collect() leaves them, read, in
        # ``map_arrays`` -- its own return value is what it was without them
        self.map_hosts, self.map_arrays = map_hosts, None

    def landed(self):
        """True once every copy has arrived; never waits."""
        return self.event is None or self.event.query()

    def buffers(self):
        return self.hosts + [h for h in (self.metric_host, self.vhost, self.lhost) if h is not None] \
            + list((self.map_hosts or {}).values())

    def _give_back(self):
        for h in self.buffers() if self.pool is not None else ():
            self.pool.give(h)

    def discard(self):
        """Wait for the copies and give the buffers back unread (a frame that is rendered again)."""
        if self.event is not None:
            self.event.synchronize()
        self._give_back()

    def collect(self):
        """Wait for the copies (the one wait per frame) and return (numpy images, metric values or None, JPEG bytes or
        None, whether the stream was longer than the cap: its remainder was then fetched here, synchronously, once);
        the buffers go back to the pool."""
        if self.event is not None:
            self.event.synchronize()
        arrs = [h.numpy().copy() if self.pool is not None else h.numpy() for h in self.hosts]
        values = None if self.metric_host is None else self.metric_host.tolist()
        if self.map_hosts is not None:
            self.map_arrays = {k: (h.numpy().copy() if self.pool is not None else h.numpy()) for k, h in self.map_hosts.items()}
        data, fell_back = None, False
        if self.vhost is not None:
            n, cap = int(self.lhost[0]), self.vhost.shape[0]
            data = self.vhost[:min(n, cap)].numpy().tobytes()
            fell_back = n > cap
            if fell_back:
                data += self.vdev[cap:n].cpu().numpy().tobytes()
        self._give_back()
        return arrs, values, data, fell_back


class FrameOutbox:
    """The way a finished frame leaves the GPU, for every loop that renders frames: ``post`` queues the copies of its
    device tensors into pooled pinned buffers on a copy stream of its own, behind ONE event, and returns a _Parcel;
    the parcel's ``collect()`` waits for that event, reads the buffers and gives them back.  On a CPU device nothing is
    copied and nothing waits."""

    def __init__(self, device):
        self.device = device
        self.stream = torch.cuda.Stream(device=device) if device.type == 'cuda' else None
        self.pool = _PinnedPool()

    def _stage(self, src):
        h = self.pool.take(src.shape, src.dtype)
        h.copy_(src, non_blocking=True)
        src.record_stream(self.stream)
        return h

    def post(self, images, metric_vec=None, video=None, maps=None):
        """``images``: uint8 tensors; ``metric_vec``: float64 vector; ``video``: (buffer, length, height, width) -- what
        JpegEncoder.encode returned for panels of height x width.  The stream's length is not known here, so its first
        min(len(buffer), video_copy_cap(height, width)) bytes and the length word travel.  ``maps``: {name: uint8
        tensor}, the geometry panels: staged behind the images, under the same event."""
        vbuf, vlen, height, width = video if video is not None else (None, None, 0, 0)
        if self.stream is None:
            return _Parcel(None, None, [im.cpu() for im in images], metric_vec, vbuf, vlen, vbuf, 0,
                           None if maps is None else {k: v.cpu() for k, v in maps.items()})
        self.stream.wait_stream(torch.cuda.current_stream(self.device))  # overlap D2H with the next frame
        with torch.cuda.stream(self.stream):
            hosts = [self._stage(im) for im in images]
            map_hosts = None if maps is None else {k: self._stage(v) for k, v in maps.items()}
            mhost = None if metric_vec is None else self._stage(metric_vec)
            vhost, lhost, cap = None, None, 0
            if vbuf is not None:
                cap = min(int(vbuf.shape[0]), video_copy_cap(height, width))
                vhost, lhost = self._stage(vbuf[:cap]), self._stage(vlen)
            event = torch.cuda.Event()
            event.record(self.stream)
        return _Parcel(self.pool, event, hosts, mhost, vhost, lhost, vbuf, cap, map_hosts)


_FRAME_KEYS = ('dst_Rs', 'dst_Ts', 'cnl_gtfms', 'dst_posevec', 'cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'bgcolor')


def with_rays(frame, device):
    """``frame`` itself when it carries ``rays``; for a camera-only frame a copy with rays, near / far and ray_mask
    from the device generator.  The rays are clipped against the POSED skeleton's bbox (freeview.py:226;
    dataset.Subject puts it in ray_bbox_*); the synthetic frames of scene.py pose nothing and use the canonical one."""
    if 'rays' in frame:
        return frame
    from . import ops
    return dict(frame, **ops.gen_rays(frame['K'], frame['E'], frame.get('ray_bbox_min_xyz', frame['cnl_bbox_min_xyz']),
                                      frame.get('ray_bbox_max_xyz', frame['cnl_bbox_max_xyz']),
                                      int(frame['img_height']), int(frame['img_width']), device=device,
                                      camera_turn=frame.get('camera_turn')))


class FramePrefetcher:
    """The DataLoader of the reference's render loops (create_dataset.py:81-85: worker processes build the per-frame
    dicts while ``run.py:240-300`` renders) for one process per GPU: a worker thread walks this rank's frame indices
    ``depth`` frames ahead of the renderer and, per frame,
      * builds ``frames[idx]`` (the host part: SMPL helpers, PNG decoding for frames that carry their image),
      * uploads it through pinned memory on a SIDE stream,
      * runs everything that needs a device round trip there as well: ray generation for camera-only frames
        (hnrf_gen_rays reads the ray count back), image undistortion / composite / resize of frames loaded by
        ``Subject.load_image_device``, the index list of the hit pixels and the truth pixels under it,
    and hands over device tensors plus the event that marks them ready.  The render stream only ever waits for that
    event: no host synchronisation is left in the loop, so the GPU renders frame n while the host prepares n+1.."""

    def __init__(self, frames, indices, device, show_truth=False, depth=4, workers=3, max_workers=6, camera=False):
        self.frames, self.indices, self.device, self.show_truth = frames, list(indices), device, show_truth
        self.camera = camera                        # hand over the frame's world-to-camera rotation too (item['M'])
        self.on_gpu = device.type == 'cuda'
        self._resident = {}
        self._lock = threading.Lock()
        self._cv = threading.Condition()
        self._done, self._next_ticket, self._stop = {}, 0, False
        self._slots = threading.Semaphore(max(1, depth))
        self.build_s, self.wait_s = [], []          # per frame: worker time to build it / time the renderer waited for it
        if self.on_gpu:
            # several frames are in the making at once: a frame's build is a chain of ~15 small launches and three
            # read-backs on a side stream, and once the renderer runs ahead (nothing in the loop waits for the GPU) each
            # of them queues behind a canonical-MLP launch that holds every SIMD for ~9 ms: 150-200 ms of latency per
            # frame, hidden by building three frames at a time (measured: profiles/r03_movement_loop.txt)
            # ... and more when that is not enough: the latency depends on the box (host speed, how the two hardware
            # queues interleave), and a faster renderer needs more frames in the making -- round 3: 3 builders fell from
            # 1.04x to 1.22x of the pure render time on one box when the render went from 97 to 87 ms, while 5 builders
            # from the start stalled single frames on another.  So the pool GROWS by one builder (and one slot of depth)
            # whenever the renderer had to wait for two frames in a row, up to max_workers.
            self._max_workers, self._waited_in_a_row = max(workers, max_workers), 0
            self._threads = [threading.Thread(target=self._work, daemon=True) for _ in range(max(1, workers))]
            for t in self._threads:
                t.start()

    # -- one frame ------------------------------------------------------------------------------------------
    def _up(self, v):
        if torch.is_tensor(v):
            return v.to(self.device, non_blocking=True)
        t = torch.as_tensor(np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v)
        if self.on_gpu and t.numel() > 0:
            return t.pin_memory().to(self.device, non_blocking=True)
        return t.to(self.device)

    def _priors(self, pri, name='priors'):
        # per-subject constant: keep it on the device while the host copy is unchanged, so that the network's
        # weight-volume cache hits by identity (no per-frame comparison / synchronisation); the same for the canonical
        # bbox, which keys the network's baked canonical grid (cfg.amd.canonical = 'baked')
        with self._lock:
            return self._priors_locked(pri, name)

    def _priors_locked(self, pri, name):
        hit = self._resident.get(name)
        if hit is not None and (hit[0] is pri or (isinstance(pri, np.ndarray) and isinstance(hit[0], np.ndarray)
                                                  and hit[0].shape == pri.shape and np.array_equal(hit[0], pri))):
            if hit[2] is not None:                                       # uploaded on another worker's stream
                torch.cuda.current_stream(self.device).wait_event(hit[2])
            return hit[1]
        t = self._up(pri)
        ev = None
        if self.on_gpu:
            ev = torch.cuda.Event()
            ev.record()
        self._resident[name] = (pri, t, ev)
        return t

    def build(self, idx):
        fr = with_rays(self.frames[idx], self.device)
        data = {k: self._up(fr[k]) for k in ('rays', 'near', 'far') + _FRAME_KEYS}
        data['motion_weights_priors'] = self._priors(fr['motion_weights_priors'])
        if cfg.get('amd', {}).get('canonical', 'mlp') == 'baked':
            for k in ('cnl_bbox_min_xyz', 'cnl_bbox_scale_xyz', 'cnl_bbox_max_xyz'):
                if k in fr:
                    data[k] = self._priors(fr[k], k)
        mask = self._up(fr['ray_mask']).reshape(-1)
        index = torch.nonzero(mask).reshape(-1)                          # (the one read-back of the frame: on this stream)
        truth = None
        if self.show_truth and fr.get('target_rgbs', None) is not None:
            truth = self._up(fr['target_rgbs'])
        elif self.show_truth and fr.get('raw_rgbs', None) is not None:   # whole image (0..1): the pixels the rays hit
            truth = self._up(fr['raw_rgbs']).reshape(-1, 3).index_select(0, index)
        item = {'idx': idx, 'data': data, 'ray_index': index, 'truth': truth,
                'W': int(fr['img_width']), 'H': int(fr['img_height'])}
        if self.camera:                                                  # (a frame without a camera: the identity)
            E = fr.get('E', None)
            item['M'] = None if E is None else self._up(np.ascontiguousarray(np.asarray(E, dtype=np.float32)[:3, :3]))
        return item

    def _work(self):
        stream = torch.cuda.Stream(device=self.device, priority=int(os.environ.get('HNRF_PREFETCH_PRIORITY', '0')))
        try:
            with torch.cuda.device(self.device), torch.cuda.stream(stream):
                while True:
                    self._slots.acquire()
                    with self._lock:
                        if self._stop or self._next_ticket >= len(self.indices):
                            return
                        ticket = self._next_ticket
                        self._next_ticket += 1
                    t0 = time.perf_counter()
                    item = self.build(self.indices[ticket])
                    ev = torch.cuda.Event()
                    ev.record(stream)
                    item['event'] = ev
                    with self._cv:
                        self.build_s.append(time.perf_counter() - t0)
                        self._done[ticket] = item
                        self._cv.notify_all()
        except BaseException as e:                                       # surfaced by the consumer
            with self._cv:
                self._done['error'] = e
                self._cv.notify_all()

    def __iter__(self):
        if not self.on_gpu:
            for idx in self.indices:
                yield self.build(idx)
            return
        main = torch.cuda.current_stream(self.device)
        for ticket in range(len(self.indices)):
            t0 = time.perf_counter()
            with self._cv:
                while ticket not in self._done and 'error' not in self._done:
                    self._cv.wait()
                if 'error' in self._done:
                    raise self._done['error']
                item = self._done.pop(ticket)
            self.wait_s.append(time.perf_counter() - t0)
            self._slots.release()
            # (the first frames always wait: the pipeline is filling)
            self._waited_in_a_row = self._waited_in_a_row + 1 if (self.wait_s[-1] > 5e-3 and ticket >= len(self._threads)) else 0
            if self._waited_in_a_row >= 2 and len(self._threads) < self._max_workers:
                self._waited_in_a_row = 0
                t = threading.Thread(target=self._work, daemon=True)
                self._threads.append(t)
                self._slots.release()                                    # one more frame in the making
                t.start()
            main.wait_event(item['event'])
            for t in list(item['data'].values()) + [item['ray_index'], item['truth'], item.get('M')]:
                if torch.is_tensor(t):
                    t.record_stream(main)                                # allocated on a side stream, consumed here
            yield item

    def close(self):
        with self._lock:
            self._stop = True
        if self.on_gpu:
            for _ in self._threads:
                self._slots.release()


METRIC_NAMES = ('psnr', 'ssim', 'lpips')

# a frame of render_frames between its launches and its hand-over: frame index, the FrameOutbox parcel of its copies, the
# prefetcher's item (to render it again), the number of frames the network's f16-range guard had watched once this one
# was queued
_InFlight = namedtuple('_InFlight', 'idx parcel item watch_id')


def select_panels(rgb8, alpha8, truth8=None, maps=None):
    """run.py:143-149 / 359-364: [render | truth if cfg.show_truth | alpha if cfg.show_alpha], as a list (arrays or
    tensors): what run._panels concatenates on the host and render_frames(video=...) on the device.  ``maps``: the
    geometry panels {name: image} of the frame (render_frames(maps=...)), appended in their order."""
    imgs = [rgb8]
    if cfg.get('show_truth', False) and truth8 is not None:
        imgs.append(truth8)
    if cfg.get('show_alpha', False):
        imgs.append(alpha8)
    if maps:
        imgs.extend(maps.values())
    return imgs


def render_frames(network, frames, rank=0, world=1, device=None, on_image=None, show_truth=False, prefetch=None,
                  metrics=None, lpips_fn=None, on_metrics=None, video=None, on_video=None, images='host', maps=None,
                  on_maps=None):
    """Render ``frames`` (sequence of per-frame input dicts, numpy or tensors) frame-sharded.

    Returns {frame_idx: uint8 rgb image on the host} for this rank's frames.  ``on_image(idx, rgb8, alpha8[,
    truth8])`` is called as images arrive (e.g. ``ImageWriter.append``); with ``show_truth`` a frame's ``target_rgbs``
    (N, 3) -- or, for camera-only frames, the pixels of its ``raw_rgbs`` image (H, W, 3) that the rays hit -- are
    unpacked next to the render (run.py:131-136) and handed over as the fourth argument.

    A frame may carry its camera instead of precomputed rays -- ``K`` (3,3), ``E`` (4,4), ``cnl_bbox_max_xyz`` next to
    ``img_width`` / ``img_height`` and no ``rays``: the rays, near/far and ray_mask are then generated on the
    device (ops.gen_rays = get_rays_from_KRT + rays_intersect_3d_bbox, freeview.py:220-230) instead of the
    per-frame numpy pass and the 32 B/ray upload.

    Frames are assembled ``prefetch`` ahead by ``FramePrefetcher`` (host work and every device read-back on a side
    stream); everything a finished frame sends to the host -- images, metric vector, JPEG stream -- is posted to one
    FrameOutbox (pinned buffers on a copy stream, one event per frame) and handed over, ``on_image`` then ``on_metrics``
    then ``on_video``, one frame late at the earliest -- after the next frame's forward has looked at this frame's
    f16-range verdict (Network.check_f16_range), so that with ``cfg.amd.on_f16_range = 'f32'`` a frame rendered out
    of range is rendered again with the exact kernels before anybody sees it.  This function keeps the device work of
    a frame, the queue of frames in flight with that handshake, the callbacks and the timing records.

    ``metrics`` (a list out of 'psnr', 'ssim', 'lpips'; GPU only, needs ``show_truth``): every frame that has its truth
    gets the metrics of its 8-bit render against its 8-bit truth ON THE DEVICE, as part of the frame's launches --
    ops.image_metrics (exact integer moments, render.metrics_u8 is its numpy statement) and, for 'lpips',
    1000 * ``lpips_fn(rgb8 / 255, truth8 / 255)`` on the device tensors (LpipsVGG.metric; the host's float32 pixels).  The values travel as one
    float64 vector through a pinned buffer behind the frame's images, under the same event, and arrive as
    ``on_metrics(idx, {name: float})`` right after that frame's ``on_image``.  Nothing of it synchronises, and a frame
    rendered again after an f16-range hit gets its metrics again.  The pixels are always divided by 255
    (MetricsWriter.normalize leaves an image whose maximum is <= 2 as it is).

    ``video`` (a video.JpegEncoder on ``device``): the frame's panels (select_panels: the choice run._panels makes on
    the host) are concatenated on the device and JPEG-encoded as part of the frame's launches.  The stream travels
    behind the images, under the same event (FrameOutbox.post: its first video_copy_cap(H, W) bytes), and arrives as
    ``on_video(idx, bytes)`` after that frame's ``on_image`` (and ``on_metrics``).  Only a stream longer than the cap
    fetches its remainder, synchronously, at hand-over (render_frames.last_video = {'frames', 'fallbacks', 'bytes',
    'cap'}: streams handed over, those that fell back, their bytes, the cap): no synchronisation enters the loop.
    A frame rendered again after an f16-range hit is encoded again.  ``images='none'`` (only with ``video``): no 8-bit
    image is copied to the host, ``on_image`` is never called and the returned dict is empty.

    ``maps`` (a list out of 'depth', 'normal', 'shaded', 'offset'; GPU only): the frame's geometry panels
    (geometry.frame_maps: the surface distance cfg.amd.maps_surface of every ray, normals as screen-space differences of
    it; three library calls in the frame's launches).  They travel behind the images, under the same event, and arrive
    as ``on_maps(idx, {name: uint8 array (H, W, 3)})`` right after that frame's ``on_image``; select_panels puts them
    behind the other panels, so ``video`` encodes them too.  The normal panel is in the camera frame of the frame's
    ``E`` (the rasteriser's shade = 'normal'); 'offset' is painted where the truth has colour when the frame has one.
    A frame rendered again after an f16-range hit gets its maps again; with ``images='none'`` they go into the video
    only.  ``on_image`` gets what it gets without maps.  With cfg.amd.maps_normals = 'gradient' the 'normal' and
    'shaded' panels are painted from density-gradient normals (Network.ray_normals, which reads one device count back per
    frame: such a loop waits for the device once per frame; 'screen', the default, never does)."""
    device = device or next(network.parameters()).device
    if images not in ('host', 'none'):
        raise ValueError("render_frames: images must be 'host' or 'none', got %r" % (images,))
    if images == 'none' and video is None:
        raise ValueError("render_frames: images = 'none' delivers nothing without a video encoder (video=...)")
    if video is not None and video.device != device:
        raise ValueError('render_frames: the video encoder is on %s, the frames on %s' % (video.device, device))
    vstat = {'frames': 0, 'fallbacks': 0, 'bytes': 0, 'cap': 0}
    render_frames.last_video = vstat
    maps = list(maps) if maps else None
    if maps is not None:
        from . import geometry
        from .config import amd_option
        maps_surface = amd_option('maps_surface', 'expected')
        geometry.check_maps(maps, maps_surface, bool(amd_option('diagnostics', True)))
        gradient_normals = amd_option('maps_normals', 'screen') == 'gradient' and ('normal' in maps or 'shaded' in maps)
        if gradient_normals and not amd_option('diagnostics', True):
            raise ValueError("cfg.amd.maps_normals = 'gradient' needs cfg.amd.diagnostics = True: the lean form returns "
                             "neither the per-sample weights nor the bone weights")
        if device.type != 'cuda':
            raise ValueError('render_frames: geometry maps need a GPU (got device %s); on the host use geometry.maps_host'
                             % device)
    metrics = list(metrics) if metrics else None
    if metrics is not None:
        bad = [k for k in metrics if k not in METRIC_NAMES]
        if bad:
            raise ValueError('render_frames: unknown metrics %r (out of %r)' % (bad, METRIC_NAMES))
        if device.type != 'cuda':
            raise ValueError('render_frames: device metrics need a GPU (got device %s); on the host use MetricsWriter.append'
                             % device)
        if 'lpips' in metrics and lpips_fn is None:
            raise ValueError('metric lpips needs an lpips_fn (LPIPS-VGG weights are not obtainable offline)')
        from . import ops
        unit = (torch.arange(256, dtype=torch.float32) / 255).to(device) if 'lpips' in metrics else None
    network.eval()
    quiet_gc()
    old = cfg.perturb
    cfg.perturb = 0.                                                     # run.py:71,215
    out = {}
    on_gpu = device.type == 'cuda'
    outbox = FrameOutbox(device)
    pending = []                                    # _InFlight records, oldest first
    guard = hasattr(network, 'check_f16_range')

    t_submit, t_wait, t_user = [], [], []           # per frame: launches queued / waiting for the image / on_image

    def deliver(entry):
        i = entry.idx
        t0 = time.perf_counter()
        arrs, values, data, fell_back = entry.parcel.collect()
        if arrs:
            out[i] = arrs[0]
        t1 = time.perf_counter()
        if on_image is not None and arrs:
            on_image(i, *arrs)
        if on_maps is not None and entry.parcel.map_arrays is not None:
            on_maps(i, entry.parcel.map_arrays)
        if on_metrics is not None and values is not None:
            on_metrics(i, dict(zip(metrics, values)))
        if data is not None:
            vstat['frames'] += 1
            vstat['fallbacks'] += fell_back
            vstat['bytes'] += len(data)
            if on_video is not None:
                on_video(i, data)
        t_wait.append(t1 - t0)
        t_user.append(time.perf_counter() - t1)

    gpu_ev = []                                     # (start, stop) events around each frame's launches, cfg.amd.loop_timing

    def render(item):
        timing = on_gpu and bool(cfg.get('amd', {}).get('loop_timing', False))
        if timing:
            gpu_ev.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            gpu_ev[-1][0].record()
        with torch.no_grad():
            res = network(**item['data'], iter_val=float(cfg.eval_iter))
        rgb8, a8, t8 = unpack_to_image(item['W'], item['H'], None, item['data']['bgcolor'] / 255., res['rgb'], res['alpha'],
                                       item['truth'], ray_index=item['ray_index'])
        mvec = None
        if metrics is not None and item['truth'] is not None:
            vals = {}
            if 'psnr' in metrics or 'ssim' in metrics:
                pm = ops.image_metrics(rgb8, t8)
                vals['psnr'], vals['ssim'] = pm[0, 0], pm[0, 1]
            if 'lpips' in metrics:
                # (a table of the host's float32 k / 255: the device divides by a scalar as a product with 1 / 255)
                vals['lpips'] = 1000 * lpips_fn(unit[rgb8.long()], unit[t8.long()]).reshape(()).to(torch.float64)
            mvec = torch.stack([vals[k] for k in metrics])
        gmaps = None
        if maps is not None:
            extra = {}
            if gradient_normals:
                # (the one place of a frame that waits for the device: Network.ray_normals reads the kept count back)
                extra['ray_normals'] = network.ray_normals(item['data'], res, iter_val=float(cfg.eval_iter))
            gm = geometry.frame_maps(item['data'], res, item['H'], item['W'], item['ray_index'], maps=maps,
                                     surface=maps_surface, M=item.get('M'), truth8=t8 if item['truth'] is not None else None,
                                     **extra)
            gmaps = {m: gm[m] for m in maps}
        vid = None
        if video is not None:
            panels = select_panels(rgb8, a8, t8 if item['truth'] is not None else None, gmaps)
            vid = video.encode(panels[0] if len(panels) == 1 else torch.cat(panels, dim=1)) + (item['H'], item['W'] * len(panels))
        if timing:
            gpu_ev[-1][1].record()
        imgs = [rgb8, a8] + ([t8] if item['truth'] is not None else [])
        parcel = outbox.post([] if images == 'none' else imgs, mvec, vid, None if images == 'none' else gmaps)
        if parcel.cap:
            vstat['cap'] = parcel.cap
        return _InFlight(item['idx'], parcel, item, network.f16_range_watched if guard else 0)

    def guard_state():
        return (network.f16_range_hits, network._mlp_mode() if hasattr(network, '_mlp_mode') else None) if guard else None

    def rerender_if_switched(before):
        """``before``: guard_state() in front of a call that looked at verdicts.  A range hit with cfg.amd.on_f16_range =
        'f32' has switched the network to the exact kernels: every frame not yet handed over was rendered with the
        clamped ones (or has no verdict yet) and is rendered again; frames handed over earlier had their verdict and
        were fine.  A hit that left the mode as it was ('ignore') renders nothing again: the frames are delivered as
        they are."""
        now = guard_state()
        if not guard or now[0] == before[0] or now[1] == before[1]:
            return
        for k, entry in enumerate(pending):
            entry.parcel.discard()
            pending[k] = render(entry.item)

    def verdicts(wait, upto=None):
        if guard:
            before = guard_state()
            network.check_f16_range(wait=wait, upto=upto)
            rerender_if_switched(before)

    def known(entry):
        return not guard or network.f16_range_checked >= entry.watch_id

    # frames in the making at once: a frame's build takes ~260 ms of LATENCY behind the render kernels, the render 85 ms;
    # three builders to start with, FramePrefetcher adds more while the renderer has to wait (14 MB of device memory per frame)
    workers = int(os.environ.get('HNRF_PREFETCH_WORKERS', 3))
    depth = int(prefetch) if prefetch is not None else workers + 1
    pre = FramePrefetcher(frames, hdist.frame_shard(len(frames), rank, world), device, show_truth=show_truth, depth=depth,
                          workers=workers, camera=maps is not None)
    try:
        for item in pre:
            before = guard_state()
            t0 = time.perf_counter()
            pending.append(render(item))                                 # (forward looks at the verdicts that have arrived)
            t_submit.append(time.perf_counter() - t0)
            rerender_if_switched(before)
            # a frame is handed over once its verdict is known and its copy has landed; at most three in flight
            while pending and (len(pending) > 3 or (known(pending[0]) and pending[0].parcel.landed())):
                if not known(pending[0]):
                    verdicts(wait=True, upto=pending[0].watch_id)              # (of the oldest frame only: the queue stays full)
                deliver(pending.pop(0))
        verdicts(wait=True)
        verdicts(wait=True)                                              # (of the frames a hit had rendered again)
        while pending:
            deliver(pending.pop(0))
    finally:
        pre.close()
        cfg.perturb = old
        ms = lambda ts: [round(t * 1e3, 2) for t in ts]
        render_frames.last_prefetch = {'workers': len(getattr(pre, '_threads', [])), 'build_ms': ms(pre.build_s), 'wait_ms': ms(pre.wait_s), 'submit_ms': ms(t_submit),
                                       'image_wait_ms': ms(t_wait), 'on_image_ms': ms(t_user)}
        if gpu_ev:
            torch.cuda.synchronize(device)
            render_frames.last_prefetch['gpu_ms'] = [round(a.elapsed_time(b), 2) for a, b in gpu_ev]
            render_frames.last_prefetch['gpu_gap_ms'] = [round(gpu_ev[i][1].elapsed_time(gpu_ev[i + 1][0]), 2)
                                                         for i in range(len(gpu_ev) - 1)]
    return out


def render_frame_ray_sharded(network, frame, rank, world, device=None, group=None):
    """ONE frame rendered by all ranks together (ray-range sharding for single-frame latency;
    frames, not rays, are the unit of render_frames).  Rank r renders the r-th contiguous range of the frame's rays --
    every rank generates the same ray list (device ray generator or the frame's own ``rays``), so no ray travels --
    and the finished (n, 4) rgb|alpha blocks are all-gathered (16 B per ray over RCCL: 3.7 MB for a 512x512 frame),
    after which every rank holds the whole image.  Returns (rgb8, alpha8) uint8 arrays on the host like
    render_frames' callbacks get them."""
    import torch.distributed as dist
    device = device or next(network.parameters()).device
    network.eval()
    fr = with_rays(frame, device)
    T = lambda v: torch.as_tensor(np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v).to(device)
    rays, near, far = T(fr['rays']), T(fr['near']), T(fr['far'])
    N = rays.shape[1]
    per = -(-N // world)                                                 # equal blocks (the last one padded)
    lo, hi = min(rank * per, N), min((rank + 1) * per, N)
    data = {k: T(fr[k]) for k in _FRAME_KEYS + ('motion_weights_priors',)}
    block = torch.zeros(per, 4, device=device)
    old = cfg.perturb
    cfg.perturb = 0.
    try:
        if hi > lo:
            with torch.no_grad():
                res = network(rays=rays[:, lo:hi].contiguous(), near=near[lo:hi].contiguous(), far=far[lo:hi].contiguous(),
                              **data, iter_val=float(cfg.eval_iter))
            block[:hi - lo, :3] = res['rgb']
            block[:hi - lo, 3] = res['alpha']
    finally:
        cfg.perturb = old
    if world > 1:
        parts = [torch.empty_like(block) for _ in range(world)]
        dist.all_gather(parts, block, group=group)
        block = torch.cat(parts, dim=0)
    block = block[:N]
    rgb8, a8, _ = unpack_to_image(int(fr['img_width']), int(fr['img_height']), T(fr['ray_mask']), data['bgcolor'] / 255.,
                                  block[:, :3], block[:, 3])
    return rgb8.cpu().numpy(), a8.cpu().numpy()
