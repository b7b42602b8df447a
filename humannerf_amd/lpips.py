"""LPIPS-VGG16 loss and metric on libhnrf's fp32-MFMA kernels (hnrf.h "LPIPS"; third_parties/lpips/lpips.py:84-129).

The pretrained weights are the user's to supply: ``LpipsVGG.load(trunk_path, lin_path)`` reads a torchvision ``vgg16``
state dict and the LPIPS package's ``weights/v0.1/vgg.pth``.  Nothing of either is bundled.  ``LpipsVGG.seeded`` builds
a random trunk of the right shapes for tests and timing; its values mean nothing as a perceptual distance.

    lp = LpipsVGG.load('vgg16-397923af.pth', 'vgg.pth')
    Trainer(network, lpips_fn=lp)                       # 1.0 * LPIPS + 0.2 * MSE, the reference's objective
    run_movement(..., metrics=['psnr', 'lpips'], lpips_fn=lp.metric)
"""
import numpy as np
import torch

from . import ops
from ._lib import HnrfError

CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)          # conv modules of vgg16().features[0..29]
POOL_BEFORE = (2, 4, 7, 10)                                          # trunk layers that a 2x2 max-pool precedes
TAP_LAYERS = tuple(l for l, _ in ops.LPIPS_TAPS)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
MIN_SIZE = 16


def seeded_trunk(seed):
    """The test trunk: per conv in order, weight = standard_normal((co,ci,3,3)) * sqrt(2 / (9 ci)), then
    bias = standard_normal(co) * 0.05, from one numpy RandomState(seed).  -> {'features.<i>.weight' / '.bias'}."""
    rs = np.random.RandomState(seed)
    state = {}
    for i, (ci, co) in zip(CONV_IDX, ops.LPIPS_CONVS):
        state['features.%d.weight' % i] = torch.from_numpy(
            (rs.standard_normal((co, ci, 3, 3)) * np.sqrt(2. / (9 * ci))).astype(np.float32))
        state['features.%d.bias' % i] = torch.from_numpy((rs.standard_normal(co) * 0.05).astype(np.float32))
    return state


def seeded_heads(seed):
    """Non-negative head vectors for timing runs without the LPIPS file (the real heads are non-negative too)."""
    rs = np.random.RandomState(seed + 7919)
    return {'lin%d.model.1.weight' % t: torch.from_numpy((rs.uniform(0, 1, (1, c, 1, 1)) / c).astype(np.float32))
            for t, (_, c) in enumerate(ops.LPIPS_TAPS)}


def _check_size(H, W):
    if H < MIN_SIZE or W < MIN_SIZE:
        raise ValueError('LPIPS-VGG needs H, W >= %d (four 2x2 pools), got %dx%d' % (MIN_SIZE, H, W))


class _LpipsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img0, img1, model):
        N, H, W, _ = img0.shape
        want = bool(ctx.needs_input_grad[0])
        packed = model.packed(img0.device)
        out, _, ws = ops.lpips_fwd(img0, img1, packed, want_grad=want)
        ctx.ws, ctx.packed, ctx.dims = (ws if want else None), packed, (N, H, W)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.ws is None:
            raise HnrfError('LPIPS backward without a saved workspace')
        N, H, W = ctx.dims
        d = ops.lpips_bwd(grad_out.contiguous().float(), ctx.packed, ctx.ws, N, H, W)
        ctx.ws = None
        return d, None, None


class LpipsVGG:
    """LPIPS(net='vgg', version='0.1') in eval mode with a frozen trunk; the gradient is with respect to the first
    argument only."""

    def __init__(self, trunk_state, lin_state):
        self.weights, self.biases, self.lins = [], [], []
        for i, (ci, co) in zip(CONV_IDX, ops.LPIPS_CONVS):
            for kind, shape, dst in (('weight', (co, ci, 3, 3), self.weights), ('bias', (co,), self.biases)):
                key = 'features.%d.%s' % (i, kind)
                v = trunk_state.get(key, trunk_state.get('%d.%s' % (i, kind)))
                if v is None:
                    raise KeyError('VGG16 trunk state dict has no %r' % key)
                if tuple(v.shape) != shape:
                    raise ValueError('%s has shape %s, expected %s' % (key, tuple(v.shape), shape))
                dst.append(v.detach().to(torch.float32).cpu().contiguous())
        for t, (_, c) in enumerate(ops.LPIPS_TAPS):
            key = 'lin%d.model.1.weight' % t
            v = lin_state.get(key)
            if v is None:
                raise KeyError('LPIPS head state dict has no %r' % key)
            if tuple(v.shape) != (1, c, 1, 1):
                raise ValueError('%s has shape %s, expected %s' % (key, tuple(v.shape), (1, c, 1, 1)))
            self.lins.append(v.detach().to(torch.float32).cpu().reshape(c).contiguous())
        self._packed = {}

    @classmethod
    def load(cls, trunk_path, lin_path):
        return cls(torch.load(trunk_path, map_location='cpu', weights_only=True),
                   torch.load(lin_path, map_location='cpu', weights_only=True))

    @classmethod
    def seeded(cls, seed, lin_state=None):
        """Seeded trunk (``seeded_trunk``) with the given heads, or seeded non-negative heads."""
        return cls(seeded_trunk(seed), lin_state if lin_state is not None else seeded_heads(seed))

    def packed(self, device):
        device = torch.device(device)
        if device.type != 'cuda':
            raise HnrfError('LPIPS runs on the GPU only: there is no CPU path')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        p = self._packed.get(device)
        if p is None:
            with torch.cuda.device(device):
                to = lambda ts: [t.to(device) for t in ts]
                p = self._packed[device] = ops.lpips_pack(to(self.weights), to(self.biases), to(self.lins))
        return p

    @staticmethod
    def _nhwc(t):
        """(N,3,H,W) -> contiguous (N,H,W,3) memory; a permuted view of such memory is taken as is."""
        t = t.permute(0, 2, 3, 1)
        return t if t.is_contiguous() else t.contiguous()

    def __call__(self, in0, in1):
        """LPIPS.forward(in0, in1): (N,3,H,W) in [-1, 1] -> (N,1,1,1)."""
        if in0.dim() != 4 or in0.shape[1] != 3 or in1.shape != in0.shape:
            raise ValueError('LPIPS takes two (N,3,H,W) tensors, got %s and %s' % (tuple(in0.shape), tuple(in1.shape)))
        if in1.requires_grad and torch.is_grad_enabled():
            raise ValueError('LPIPS differentiates with respect to its first argument only')
        _check_size(in0.shape[2], in0.shape[3])
        if not (in0.is_cuda and in1.is_cuda):
            raise HnrfError('LPIPS runs on the GPU only: there is no CPU path')
        a, b = self._nhwc(in0.float()), self._nhwc(in1.detach().float())
        with torch.cuda.device(a.device):
            return _LpipsFn.apply(a, b, self).reshape(-1, 1, 1, 1)

    def layers(self, in0, in1):
        """The true per-tap values (5, N) (the reference's retPerLayer list is aliased to the total)."""
        _check_size(in0.shape[2], in0.shape[3])
        a, b = self._nhwc(in0.detach().float()), self._nhwc(in1.detach().float())
        with torch.cuda.device(a.device):
            return ops.lpips_fwd(a, b, self.packed(a.device), want_layers=True)[1]

    def metric(self, pred, target, device=None):
        """LpipsComputer.compute_lpips: (H,W,3) or (N,H,W,3) in [0, 1], CPU or GPU -> the mean value (0-dim tensor)."""
        if isinstance(pred, np.ndarray):
            pred = torch.from_numpy(pred)
        if isinstance(target, np.ndarray):
            target = torch.from_numpy(target)
        if pred.dim() == 3:
            pred, target = pred[None], target[None]
        dev = torch.device(device) if device is not None else (pred.device if pred.is_cuda else torch.device('cuda'))
        with torch.no_grad():
            p = pred.detach().to(dev, torch.float32).permute(0, 3, 1, 2) * 2. - 1.
            t = target.detach().to(dev, torch.float32).permute(0, 3, 1, 2) * 2. - 1.
            return torch.mean(self(p, t))
