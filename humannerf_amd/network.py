"""``Network`` -- drop-in for the reference's core/nets/human_nerf/network.py.

Same constructor (no arguments, reads the global ``cfg``), same ``forward``
keyword interface and output keys, same ``state_dict`` key names (including
the ``.module.`` infix nn.DataParallel inserted in the reference -- checkpoint
and optimizer-group compatibility), same attribute names the
optimizer routes learning rates by (optimizer.py:9-34).  Select it with
``network_module: 'humannerf_amd.network'`` (create_network.py:6-15 loads the
dotted path with imp.load_source).

What differs is everything underneath: the per-sample work (sampling, LBS warp,
both MLPs, compositing) runs in the hand-written HIP kernels of libhnrf.so, one
process per GPU, whole renderer replicated on every GPU.  The reference's
primary/secondary GPU split and its per-call parameter broadcast
(network.py:68-72,115-119) do not exist here; ``deploy_mlps_to_secondary_gpus``
is kept as a no-op.  Per-frame work that is a few KFLOP (pose refinement,
kinematic chain, 4x4 inverses) and the once-per-frame weight-volume decoder stay
in PyTorch-ROCm.

Only the default-config branches are implemented; anything else raises.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .autograd import RenderRays, ViewBias
from .config import cfg, amd_option, check_amd_options
from .kept import Kept, _resident, _still_resident     # noqa: F401  (the rule keeps its name here for its importers)
from .range_guard import ActivationRangeError, InferenceRangeGuard     # noqa: F401  (the error's importers look here)

SMPL_PARENT = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16,
               17, 18, 19, 20, 21]          # core/utils/network_util.py:91-94


# --------------------------------------------------------------------------- init
def _xavier_like(layer, next_act):
    """Initialisation with the distribution of the reference's initseq/initmod
    (core/utils/network_util.py:163-290): U(+-sqrt(3) gain sqrt(2/((n_in+n_out) k)))
    with k = kernel volume / stride volume for transposed convs, zero bias, and the
    2x2x2 block-replicated kernel for stride-2 ConvTranspose3d."""
    if isinstance(next_act, nn.ReLU):
        gain = math.sqrt(2.0)
    elif isinstance(next_act, nn.LeakyReLU):
        gain = math.sqrt(2.0 / (1.0 + next_act.negative_slope ** 2))
    else:
        gain = 1.0
    if isinstance(layer, nn.Linear):
        fan = layer.in_features + layer.out_features
    elif isinstance(layer, nn.ConvTranspose3d):
        k = layer.kernel_size[0] * layer.kernel_size[1] * layer.kernel_size[2]
        k //= layer.stride[0] * layer.stride[1] * layer.stride[2]
        fan = (layer.in_channels + layer.out_channels) * k
    else:
        return
    bound = gain * math.sqrt(2.0 / fan) * math.sqrt(3.0)
    with torch.no_grad():
        layer.weight.uniform_(-bound, bound)
        if layer.bias is not None:
            layer.bias.zero_()
        if isinstance(layer, nn.ConvTranspose3d):
            w = layer.weight
            base = w[:, :, 0::2, 0::2, 0::2].clone()
            for a in (0, 1):
                for b in (0, 1):
                    for c in (0, 1):
                        w[:, :, a::2, b::2, c::2] = base


def _init_sequence(mods):
    mods = list(mods)
    for cur, nxt in zip(mods, mods[1:] + [None]):
        _xavier_like(cur, nxt)


def _tiny_last_layer(layer, val=1e-5):
    with torch.no_grad():
        layer.weight.uniform_(-val, val)
        layer.bias.zero_()


class _Replicated(nn.Module):
    """Stands where the reference has nn.DataParallel(mlp): only there to keep
    the ``<name>.module.<...>`` parameter names."""

    def __init__(self, module):
        super().__init__()
        self.module = module


# --------------------------------------------------------------------------- parts
class _NonRigidParams(nn.Module):
    """Parameters of NonRigidMotionMLP (non_rigid_motion_mlps/mlp_offset.py:9-71)."""

    def __init__(self, pos_embed_size, condition_code_size, mlp_width, mlp_depth, skips):
        super().__init__()
        if not (pos_embed_size == 36 and condition_code_size == 69 and mlp_width == 128
                and mlp_depth == 6 and list(skips) == [4]):
            raise NotImplementedError('only the default non-rigid MLP (6x128, skip 4, PE36, cond 69) is built')
        mods = [nn.Linear(pos_embed_size + condition_code_size, mlp_width), nn.ReLU()]
        for i in range(1, mlp_depth):
            n_in = mlp_width + pos_embed_size if i in skips else mlp_width
            mods += [nn.Linear(n_in, mlp_width), nn.ReLU()]
        mods += [nn.Linear(mlp_width, 3)]
        self.block_mlps = nn.ModuleList(mods)
        _init_sequence(self.block_mlps)
        _tiny_last_layer(self.block_mlps[-1])          # mlp_offset.py:60-66

    def linears(self):
        return [m for m in self.block_mlps if isinstance(m, nn.Linear)]


class _CanonicalParams(nn.Module):
    """Parameters of CanonicalMLP default branch (canonical_mlps/mlp_rgb_sigma.py:64-99)."""

    def __init__(self, input_ch, mlp_depth, mlp_width, skips, n_heads=1, view_ch=0):
        """``view_ch`` > 0: the view branch (mlp_rgb_sigma.py:85-96) on a direction embedding of that many columns --
        output_linear_density, output_linear_rgb_1, output_linear_rgb_2 in the place of output_linear, under the
        reference's names and with nn.Linear's default initialisation (initseq touches pts_linears only there)."""
        super().__init__()
        if not (input_ch == 63 and mlp_depth == 8 and mlp_width == 256 and list(skips) == [4]):
            raise NotImplementedError('only the default canonical MLP (8x256, skip 4, PE63) is built')
        mods = [nn.Linear(input_ch, mlp_width), nn.ReLU()]
        for i in range(mlp_depth - 1):
            n_in = mlp_width + input_ch if i in skips else mlp_width
            mods += [nn.Linear(n_in, mlp_width), nn.ReLU()]
        self.pts_linears = nn.ModuleList(mods)
        _init_sequence(self.pts_linears)
        self.view_ch = int(view_ch)
        if self.view_ch:
            assert n_heads == 1, 'Unsupported multihead+view-dependent rgb'          # (mlp_rgb_sigma.py:86)
            self.output_linear_density = nn.Sequential(nn.Linear(mlp_width, 1))
            self.output_linear_rgb_1 = nn.Sequential(nn.Linear(mlp_width, mlp_width))
            self.output_linear_rgb_2 = nn.Sequential(nn.Linear(mlp_width + self.view_ch, mlp_width), nn.Linear(mlp_width, 3))
            return
        # multihead, head_depth 1 (mlp_rgb_sigma.py:114-115): head g is rows 4g .. 4g+3
        self.output_linear = nn.Sequential(nn.Linear(mlp_width, 4 * n_heads))
        _init_sequence(self.output_linear)

    def trunk(self):
        return [m for m in self.pts_linears if isinstance(m, nn.Linear)]

    def linears(self):
        """The nine layers every kernel knows.  With the view branch there is no ninth: its place is taken by the folded
        head (fold_view_branch), which Network states once (_cnl_layers)."""
        if self.view_ch:
            raise RuntimeError('the canonical MLP has a view branch: its head is folded from view_layers() '
                               '(network.fold_view_branch), there is no output_linear')
        return self.trunk() + [self.output_linear[0]]

    def view_layers(self):
        """output_linear_density.0, output_linear_rgb_1.0, output_linear_rgb_2.0, output_linear_rgb_2.1"""
        return [self.output_linear_density[0], self.output_linear_rgb_1[0], self.output_linear_rgb_2[0],
                self.output_linear_rgb_2[1]]


def fold_view_branch(density, rgb_1, rgb_2a, rgb_2b, dtype=None):
    """The view branch of the reference's CanonicalMLP has no non-linearity behind the trunk output h
    (mlp_rgb_sigma.py:168-178):  density = Wd h + bd,  rgb = W3 (W2 [W1 h + b1 ; e(d)] + b2) + b3.  So
        raw = [A ; Wd] h + [c ; bd] + (B e(d), 0),   A = W3 W2[:, :n] W1,  B = W3 W2[:, n:],  c = W3 (W2[:, :n] b1 + b2) + b3.
    Returns (head weight (4, n) = A | Wd, head bias (4,) = c | bd, B (3, view_ch)) from the four layers (modules, or
    (weight, bias) pairs), in plain torch ops: under autograd the gradient goes back to the four layers.  ``dtype``: the
    arithmetic (inference folds in float64 and rounds once); None = the parameters' own."""
    pair = lambda l: (l.weight, l.bias) if hasattr(l, 'weight') else l
    cast = (lambda t: t) if dtype is None else (lambda t: t.to(dtype))
    (Wd, bd), (W1, b1), (W2, b2), (W3, b3) = [tuple(cast(t) for t in pair(l)) for l in (density, rgb_1, rgb_2a, rgb_2b)]
    n = W1.shape[0]
    W32 = W3 @ W2[:, :n]
    A, B = W32 @ W1, W3 @ W2[:, n:]
    c = W32 @ b1 + W3 @ b2 + b3
    return torch.cat([A, Wd], dim=0), torch.cat([c, bd.reshape(1)], dim=0), B.contiguous()


def view_embedding(dirs, bands):
    """e(d) of the reference (network.py:499-507 + fourier.py): normalize(d), then per band sin(2^k n), cos(2^k n).
    dirs (..., 3) -> (..., 3 + 6 bands), in dirs' dtype: the host statement of what hnrf_view_bias_fwd embeds."""
    n = F.normalize(dirs, dim=-1)
    parts = [n]
    for k in range(bands):
        parts += [torch.sin(n * (2.0 ** k)), torch.cos(n * (2.0 ** k))]
    return torch.cat(parts, dim=-1)


_POINT_CONV = True       # (A/B switch of the 1x1x1 special case, profiles/tools/ab_pose.py)


class _ConvT3dK4S2P1(torch.autograd.Function):
    """Forward: the library's transposed convolution.  Backward: two plain GEMMs on the weight's NATIVE layout.

    With col[i, (co, k)] = g[co, 2 i - 1 + k] (the 4x4x4 stride-2 windows of the padded output gradient, one
    strided-view copy) the adjoint of ConvTranspose3d(4, 2, 1) is
        dx[i, ci]      = sum_(co,k) col[i, (co,k)] W[ci, (co,k)]          (D H W x 64 Cout) @ (64 Cout x Cin)
        dW[ci, (co,k)] = sum_i      x[i, ci]       col[i, (co,k)]          (Cin x D H W) @ (D H W x 64 Cout)
    -- no permuted copy of the 254 MB of decoder weights.  MIOpen has no tuned backward for these batch-1
    transposed 3-D convolutions: its solver search runs seconds of naive kernels on a fresh machine and settles
    on anything from 4 to 13 ms per training step for 20 GFLOP of work.

    A 1x1x1 input (the decoder's first layer: 1024 -> 512 channels, 33.5 M of the network's 64.4 M parameters) only
    ever meets the central 2x2x2 taps of the 4x4x4 kernel: out[co, o] = sum_ci x[ci] W[ci, co, o + 1].  That layer
    is a GEMV on those taps (16.8 MB gathered from the 134 MB tensor) instead of a pass over all 64 taps, forward and
    backward; the other 56 taps get the zero gradient they always had."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.point = _POINT_CONV and tuple(x.shape[2:]) == (1, 1, 1)
        if ctx.point:
            cin, cout = weight.shape[:2]
            wc = weight[:, :, 1:3, 1:3, 1:3].reshape(cin, cout * 8)          # (strided gather, contiguous copy)
            ctx.save_for_backward(x, wc)
            out = (x.reshape(1, cin) @ wc).reshape(1, cout, 2, 2, 2)
            return out + bias.reshape(1, cout, 1, 1, 1) if bias is not None else out
        ctx.save_for_backward(x, weight)
        if x.is_cuda and x.dtype == torch.float32 and x.shape[0] == 1:
            # GEMM on the native weight layout + the fold kernel of libhnrf (the adjoint of the backward's unfold): the same
            # two launches on every box, where MIOpen's choice for these batch-1 layers ranged from 0.15 to 1.3 ms per step
            _, cin, D, H, W = x.shape
            cout = weight.shape[1]
            col = x[0].reshape(cin, D * H * W).t() @ weight.reshape(cin, cout * 64)
            return ops.deconv_fold(col.contiguous(), None if bias is None else bias.detach().contiguous(), cout, D, H, W)
        return F.conv_transpose3d(x, weight, bias, stride=2, padding=1)

    @staticmethod
    def backward(ctx, g):
        if ctx.point:
            x, wc = ctx.saved_tensors
            cin, cout = wc.shape[0], wc.shape[1] // 8
            gm = g.reshape(1, cout * 8)
            dx = (gm @ wc.t()).reshape(1, cin, 1, 1, 1)
            dw = x.new_zeros(cin, cout, 4, 4, 4)
            dw[:, :, 1:3, 1:3, 1:3] = (x.reshape(cin, 1) @ gm).reshape(cin, cout, 2, 2, 2)
            return dx, dw, g[0].sum(dim=(1, 2, 3))
        x, weight = ctx.saved_tensors
        _, cin, D, H, W = x.shape
        cout = weight.shape[1]
        g3 = g[0]
        col = F.pad(g3, (1, 1, 1, 1, 1, 1)).unfold(1, 4, 2).unfold(2, 4, 2).unfold(3, 4, 2)   # (Cout, D, H, W, 4,4,4)
        col = col.permute(1, 2, 3, 0, 4, 5, 6).reshape(D * H * W, cout * 64)
        wm = weight.reshape(cin, cout * 64)
        xm = x[0].reshape(cin, D * H * W)
        dx = (col @ wm.t()).t().reshape(1, cin, D, H, W)
        dw = (xm @ col).reshape(cin, cout, 4, 4, 4)
        return dx, dw, g3.sum(dim=(1, 2, 3))


def conv_transpose3d_k4s2p1(x, weight, bias):
    """nn.ConvTranspose3d(kernel 4, stride 2, padding 1) of a batch-1 volume, x (1, Cin, D, H, W), with the
    GEMM backward above."""
    return _ConvT3dK4S2P1.apply(x, weight, bias)


class _PointDeconv(nn.Module):
    """ConvTranspose3d(cin, cout, 4, 2, 1) whose input is always 1x1x1: the decoder's first layer (network_util.py:30-33),
    33.5 M of the reference's 64.4 M parameters.  Such a layer only ever meets the central 2x2x2 taps of its kernel
    (out[co, o] = sum_ci x[ci] W[ci, co, o + 1]); the other 56 taps of every (ci, co) pair receive the gradient zero, so
    Adam's moments for them stay zero and so does their update: they keep their initial / loaded values for ever.
    Here the PARAMETER ``weight`` therefore holds the central taps only, (cin, cout, 2, 2, 2) -- it is what the GEMV reads
    and what autograd and the optimizer see (16.8 MB instead of 134 MB: no strided gather in the forward, no 134 MB
    zero-fill + scatter in the backward, an eighth of the optimizer's stream; bit-identical updates) -- and the full tensor
    lives on as the buffer ``weight_rest``.  ``state_dict`` / ``load_state_dict`` keep the reference's key and
    shape: 'block_conv.0.weight' (cin, cout, 4, 4, 4) with the central taps inserted / split off; GroupedAdam does the
    same for the moments in optimizer checkpoints (``hnrf_full_shape`` marks the parameter)."""

    def __init__(self, conv):
        super().__init__()
        assert isinstance(conv, nn.ConvTranspose3d) and conv.kernel_size == (4, 4, 4) and conv.stride == (2, 2, 2)
        self.in_channels, self.out_channels = conv.in_channels, conv.out_channels
        full = conv.weight.data
        self.weight = nn.Parameter(full[:, :, 1:3, 1:3, 1:3].contiguous())
        self.weight.hnrf_full_shape = tuple(full.shape)
        self.bias = nn.Parameter(conv.bias.data.clone())
        self.register_buffer('weight_rest', full.clone(), persistent=False)

    def full_weight(self):
        return expand_central_taps(self.weight.detach(), self.weight_rest)

    def forward(self, x):
        cin, cout = self.in_channels, self.out_channels
        assert tuple(x.shape) == (1, cin, 1, 1, 1)
        out = (x.reshape(1, cin) @ self.weight.reshape(cin, cout * 8)).reshape(1, cout, 2, 2, 2)
        return out + self.bias.reshape(1, cout, 1, 1, 1)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        destination[prefix + 'weight'] = self.full_weight()
        destination[prefix + 'bias'] = self.bias if keep_vars else self.bias.detach()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        w = state_dict.get(prefix + 'weight')
        if w is not None and tuple(w.shape) == tuple(self.weight.hnrf_full_shape):
            with torch.no_grad():
                self.weight_rest.copy_(w)
                self.weight.copy_(w[:, :, 1:3, 1:3, 1:3])
            state_dict = {k: v for k, v in state_dict.items() if k != prefix + 'weight'}
            state_dict[prefix + 'weight'] = self.weight.detach().clone()
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


def expand_central_taps(central, rest=None):
    """(cin, cout, 2, 2, 2) central taps -> the reference's (cin, cout, 4, 4, 4) tensor: ``rest`` (or zeros: gradients,
    optimizer moments) with the central taps replaced."""
    cin, cout = central.shape[:2]
    full = rest.clone() if rest is not None else central.new_zeros(cin, cout, 4, 4, 4)
    full[:, :, 1:3, 1:3, 1:3] = central
    return full


def full_gradient(param):
    """``param.grad`` in the reference's shape (a compact decoder parameter's gradient expanded with zeros)."""
    g = param.grad
    if g is not None and getattr(param, 'hnrf_full_shape', None) is not None and tuple(g.shape) != tuple(param.hnrf_full_shape):
        return expand_central_taps(g)
    return g


class _ConvDecoder3D(nn.Module):
    """core/utils/network_util.py:12-50."""

    def __init__(self, embedding_size, volume_size, voxel_channels):
        super().__init__()
        self.block_mlp = nn.Sequential(nn.Linear(embedding_size, 1024), nn.LeakyReLU(0.2))
        convs, cin, cout = [], 1024, 512
        for _ in range(int(math.log2(volume_size)) - 1):
            convs += [nn.ConvTranspose3d(cin, cout, 4, 2, 1), nn.LeakyReLU(0.2)]
            if cin == cout:
                cout = cin // 2
            else:
                cin = cout
        convs.append(nn.ConvTranspose3d(cin, voxel_channels, 4, 2, 1))
        self.block_conv = nn.Sequential(*convs)
        _init_sequence(self.block_mlp)
        _init_sequence(self.block_conv)
        if _POINT_CONV:
            self.block_conv[0] = _PointDeconv(self.block_conv[0])     # (after the reference's initialisation of all 64 taps)

    def forward(self, embedding):
        h = self.block_mlp(embedding).view(-1, 1024, 1, 1, 1)
        for m in self.block_conv:                                   # parameters live in the reference's modules
            h = conv_transpose3d_k4s2p1(h, m.weight, m.bias) if isinstance(m, nn.ConvTranspose3d) else m(h)
        return h


class MotionWeightVolumeDecoder(nn.Module):
    """mweight_vol_decoders/deconv_vol_decoder.py:8-33 (9 GFLOP once per frame against 40 TFLOP of per-sample
    work: stays PyTorch, with the transposed convolutions as batched GEMMs)."""

    def __init__(self, embedding_size=256, volume_size=32, total_bones=24):
        super().__init__()
        self.const_embedding = nn.Parameter(torch.randn(embedding_size), requires_grad=True)
        self.decoder = _ConvDecoder3D(embedding_size, volume_size, total_bones + 1)

    def forward(self, motion_weights_priors, **_):
        dec = self.decoder(self.const_embedding[None, ...])
        return F.softmax(dec + torch.log(motion_weights_priors), dim=1)


class BodyPoseRefiner(nn.Module):
    """pose_decoders/mlp_delta_body_pose.py:7-41."""

    def __init__(self, embedding_size=69, mlp_width=256, mlp_depth=4, total_bones=24):
        super().__init__()
        mods = [nn.Linear(embedding_size, mlp_width), nn.ReLU()]
        for _ in range(mlp_depth - 1):
            mods += [nn.Linear(mlp_width, mlp_width), nn.ReLU()]
        self.total_bones = total_bones - 1
        mods += [nn.Linear(mlp_width, 3 * self.total_bones)]
        self.block_mlps = nn.Sequential(*mods)
        _init_sequence(self.block_mlps)
        _tiny_last_layer(self.block_mlps[-1])

    def rvec(self, pose_input):
        """The MLP alone: axis-angle corrections (N * 23, 3).  One pose vector on the GPU: the single-workgroup kernels
        of libhnrf (hnrf_pose_mlp_fwd / _bwd) instead of ~30 GEMV / bias / ReLU launches per training step."""
        linears = [m for m in self.block_mlps if isinstance(m, nn.Linear)]
        if pose_input.is_cuda and pose_input.numel() == linears[0].in_features and \
                all(max(m.in_features, m.out_features) <= 256 for m in linears) and len(linears) <= 9:
            params = [p for m in linears for p in (m.weight, m.bias)]
            return _PoseMLP.apply(pose_input.reshape(-1), *params).view(-1, 3)
        return self.block_mlps(pose_input).view(-1, 3)

    def forward(self, pose_input):
        rvec = self.rvec(pose_input)
        return {'Rs': rodrigues(rvec).view(-1, self.total_bones, 3, 3),
                'rvec': rvec.view(-1, self.total_bones, 3)}


class _PoseMLP(torch.autograd.Function):
    """x (n_in,), W0, b0, W1, b1, ... -> MLP(x) on hnrf_pose_mlp_fwd; backward on hnrf_pose_mlp_bwd."""

    @staticmethod
    def forward(ctx, x, *params):
        x = x.contiguous().float()
        weights = [p.contiguous() for p in params[0::2]]
        biases = [p.contiguous() for p in params[1::2]]
        out, saved = ops.pose_mlp_fwd(x, weights, biases)
        ctx.save_for_backward(x, saved, *weights, *biases)
        ctx.n_layers = len(weights)
        return out

    @staticmethod
    def backward(ctx, g):
        x, saved = ctx.saved_tensors[:2]
        L = ctx.n_layers
        weights, biases = list(ctx.saved_tensors[2:2 + L]), list(ctx.saved_tensors[2 + L:2 + 2 * L])
        dW, db, d_x = ops.pose_mlp_bwd(g.contiguous(), x, weights, biases, saved, want_dx=ctx.needs_input_grad[0])
        grads = [None] * (2 * L)
        grads[0::2], grads[1::2] = dW, db
        return (d_x, *grads)


def rodrigues(rvec):
    """Batch Rodrigues with theta = sqrt(1e-5 + |r|^2) (network_util.py:57-83)."""
    theta = torch.sqrt(1e-5 + torch.sum(rvec ** 2, dim=1))
    r = rvec / theta[:, None]
    c, s = torch.cos(theta), torch.sin(theta)
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    oc = 1. - c
    return torch.stack((x * x + (1. - x * x) * c, x * y * oc - z * s, x * z * oc + y * s,
                        x * y * oc + z * s, y * y + (1. - y * y) * c, y * z * oc - x * s,
                        x * z * oc - y * s, y * z * oc + x * s, z * z + (1. - z * z) * c), dim=1).view(-1, 3, 3)


class _MotionBasis(torch.autograd.Function):
    """MotionBasisComputer.forward (network_util.py:125-156) and its backward on libhnrf's single-wave kernels
    (hnrf_motion_basis_fwd / _bwd) instead of ~120 tiny PyTorch launches per training step."""

    @staticmethod
    def forward(ctx, dst_Rs, dst_Ts, cnl_gtfms, rvec=None):
        dst_Rs, dst_Ts, cnl_gtfms = dst_Rs.contiguous(), dst_Ts.contiguous(), cnl_gtfms.contiguous()
        rvec = rvec.contiguous() if rvec is not None else None
        need = dst_Rs.requires_grad or dst_Ts.requires_grad or (rvec is not None and rvec.requires_grad)
        Rs, Ts, saved = ops.motion_basis_fwd(dst_Rs, dst_Ts, cnl_gtfms, want_saved=need, rvec=rvec)
        ctx.refined = rvec is not None
        if need:
            ctx.save_for_backward(dst_Rs, dst_Ts, cnl_gtfms, saved, *((rvec,) if ctx.refined else ()))
        return Rs, Ts

    @staticmethod
    def backward(ctx, g_Rs, g_Ts):
        dst_Rs, dst_Ts, cnl_gtfms, saved = ctx.saved_tensors[:4]
        rvec = ctx.saved_tensors[4] if ctx.refined else None
        out = ops.motion_basis_bwd(g_Rs.contiguous(), g_Ts.contiguous(), dst_Rs, dst_Ts, cnl_gtfms, saved, rvec=rvec)
        return out[0], out[1], None, (out[2] if ctx.refined else None)


def motion_basis(dst_Rs, dst_Ts, cnl_gtfms, rvec=None):
    """MotionBasisComputer.forward for one frame: (B,3,3),(B,3),(B,4,4) -> (B,3,3),(B,3).  ``rvec`` (B-1,3): the pose
    refinement dst_Rs[1:] <- dst_Rs[1:] Rodrigues(rvec) (network.py:677-688) applied first.  On the GPU: the fused
    kernel; the torch restatement below it serves CPU-side checks only."""
    if dst_Rs.is_cuda and dst_Rs.shape[0] == 24:
        return _MotionBasis.apply(dst_Rs, dst_Ts, cnl_gtfms, rvec)
    if rvec is not None:
        dst_Rs = torch.cat([dst_Rs[0:1], torch.matmul(dst_Rs[1:], rodrigues(rvec))], dim=0)
    return motion_basis_torch(dst_Rs, dst_Ts, cnl_gtfms)


def motion_basis_torch(dst_Rs, dst_Ts, cnl_gtfms):
    """MotionBasisComputer.forward (network_util.py:125-156) for one frame in plain torch ops:
    (B,3,3),(B,3),(B,4,4) -> (B,3,3),(B,3)."""
    B = dst_Rs.shape[0]
    G = torch.zeros(B, 4, 4, dtype=dst_Rs.dtype, device=dst_Rs.device)
    G[:, :3, :3] = dst_Rs
    G[:, :3, 3] = dst_Ts
    G[:, 3, 3] = 1.0
    chain = [G[0]]
    for i in range(1, B):
        chain.append(torch.matmul(chain[SMPL_PARENT[i]], G[i]))
    # inv_ex without the error check: torch.inverse reads the LAPACK status back to the host, a device
    # synchronisation per frame that exposes the launch latency of everything queued behind it
    f_mtx = torch.matmul(cnl_gtfms, torch.linalg.inv_ex(torch.stack(chain), check_errors=False).inverse)
    return f_mtx[:, :3, :3].contiguous(), f_mtx[:, :3, 3].contiguous()


def hann_window_weights(iter_val, multires, kick_in_iter, full_band_iter):
    """Per-band weights of the coarse-to-fine window (hannw_fourier.py:26-40),
    fp32 on the host like the reference's float32 constants."""
    kick = torch.tensor(float(kick_in_iter), dtype=torch.float32)
    t = torch.clamp(torch.tensor(float(iter_val), dtype=torch.float32) - kick, min=0.)
    N = full_band_iter - kick_in_iter
    alpha = torch.tensor(float(multires), dtype=torch.float32) if N == 0 else multires * t / N
    k = torch.arange(multires, dtype=torch.float32)
    return (1. - torch.cos(math.pi * torch.clamp(alpha - k, min=0., max=1.))) / 2.


def _vec3(a, dev):
    return torch.as_tensor(a).to(device=dev, dtype=torch.float32).reshape(3).contiguous()


# --------------------------------------------------------------------------- network
def _node(root, path, default=None):
    cur = root
    for part in path.split('.'):
        if cur is None or not hasattr(cur, 'get'):
            return default
        cur = cur.get(part, None)
    return default if cur is None else cur


# every switch of the reference's Network.__init__ / CanonicalMLP / NonRigidMotionMLP constructors that selects a
# branch this build does not have (network.py:36-159, mlp_rgb_sigma.py:14-130, mlp_offset.py:9-71), with the only
# value that is built.  Module paths are compared by their last component.
_BUILT_BRANCHES = (
    ('non_rigid_motion_model', 'mlp'),
    ('canonical_mlp.view_dir', False), ('canonical_mlp.pose_color', 'wo'),
    ('canonical_mlp.mlp_depth_plus', 0), ('canonical_mlp.last_linear_scale', 1), ('canonical_mlp.i_embed', 0),
    ('canonical_mlp.time_input', False), ('canonical_mlp.module', 'mlp_rgb_sigma'),
    ('non_rigid_motion_mlp.mlp_depth_plus', 0), ('non_rigid_motion_mlp.last_linear_scale', 1),
    ('non_rigid_motion_mlp.i_embed', 0), ('non_rigid_motion_mlp.time_input', False),
    ('non_rigid_motion_mlp.pose_input', True), ('non_rigid_motion_mlp.multihead.enable', False),
    ('non_rigid_motion_mlp.module', 'mlp_offset'),
    ('rgb_history.last_num', 0), ('posevec.type', 'axis_angle'), ('condition_code.type', 'global'),
    ('embedder.module', 'fourier'), ('non_rigid_embedder.module', 'hannw_fourier'),
    ('mweight_volume.module', 'deconv_vol_decoder'), ('pose_decoder.module', 'mlp_delta_body_pose'),
)


VIEW_BANDS_MIN, VIEW_BANDS_MAX = 1, 10   # multires_dir of the view branch (hnrf_view.h)


def view_dir_bands(config):
    """Bands L of the direction embedding (3 + 6 L columns) when ``config`` selects view-dependent colour AND opts in
    (``canonical_mlp.view_dir`` with ``amd.view_dir``), else 0.  check_config_is_built says which values are built."""
    if not (bool(_node(config, 'canonical_mlp.view_dir', False)) and bool(_node(config, 'amd.view_dir', False))):
        return 0
    return _node(config, 'canonical_mlp.multires_dir', 4)


HEADS_MIN, HEADS_MAX = 2, 8         # the canonical MLP's head layer is one 32-row MFMA tile: up to 8 heads x 4 outputs


def canonical_head_num(config):
    """Number of heads of the canonical MLP ``config`` selects: 0 without ``canonical_mlp.multihead.enable``, else the
    top-level ``multihead.head_num``.  check_config_is_built says which values are built."""
    if not bool(_node(config, 'canonical_mlp.multihead.enable', False)):
        return 0
    return _node(config, 'multihead.head_num', None)


def check_config_is_built(config):
    """Raise unless ``config`` selects exactly the default-config branches of the reference network, or those with a
    multi-head canonical MLP of head depth 1 (``canonical_mlp.multihead.enable`` with a top-level ``multihead.head_num``
    of 2..8, inference only).  A checkpoint trained with any other setting (e.g. ``mlp_depth_plus: 2``) has extra /
    different tensors that a non-strict ``load_state_dict`` would drop silently, and the render would be wrong without
    an error."""
    bad = []
    if bool(_node(config, 'canonical_mlp.multihead.enable', False)):
        heads = canonical_head_num(config)
        if isinstance(heads, bool) or not isinstance(heads, int) or not HEADS_MIN <= heads <= HEADS_MAX:
            bad.append('canonical_mlp.multihead.enable = True with multihead.head_num = %r (built: %d..%d)'
                       % (heads, HEADS_MIN, HEADS_MAX))
        depth = _node(config, 'canonical_mlp.multihead.head_depth', 1)
        if depth != 1:
            bad.append('canonical_mlp.multihead.head_depth = %r (built: 1)' % (depth,))
    # view-dependent colour: built behind the opt-in amd.view_dir (DESIGN.md section 4 "View-dependent colour")
    view = bool(_node(config, 'canonical_mlp.view_dir', False)) and bool(_node(config, 'amd.view_dir', False))
    if view:
        if bool(_node(config, 'canonical_mlp.multihead.enable', False)):
            bad.append('canonical_mlp.view_dir = True with canonical_mlp.multihead.enable = True (the reference refuses '
                       'multihead + view-dependent rgb itself)')
        embed = _node(config, 'canonical_mlp.view_embed', 'mlp')
        if embed != 'mlp':
            bad.append("canonical_mlp.view_embed = %r (built: 'mlp'; 'vocab' is not)" % (embed,))
        L = view_dir_bands(config)
        if isinstance(L, bool) or not isinstance(L, int) or not VIEW_BANDS_MIN <= L <= VIEW_BANDS_MAX:
            bad.append('canonical_mlp.multires_dir = %r (built: an int in %d..%d)' % (L, VIEW_BANDS_MIN, VIEW_BANDS_MAX))
    for path, want in _BUILT_BRANCHES:
        if view and path == 'canonical_mlp.view_dir':
            continue
        have = _node(config, path, want)
        if path.endswith('.module'):
            have = str(have).split('.')[-1]
        if isinstance(want, bool):
            have = bool(have)
        if have != want:
            bad.append('%s = %r (built: %r%s)' % (path, have, want, ', or True with the opt-in cfg.amd.view_dir = True'
                                                  if path == 'canonical_mlp.view_dir' else ''))
    if bad:
        raise NotImplementedError('configuration selects branches outside the hot path this build implements '
                                  '(SURVEY.md section 2.1): ' + '; '.join(bad))


class Network(nn.Module):
    def __init__(self):
        super().__init__()
        check_config_is_built(cfg)
        cm, nr = cfg.canonical_mlp, cfg.non_rigid_motion_mlp
        self.total_bones = cfg.total_bones

        self.mweight_vol_decoder = MotionWeightVolumeDecoder(
            embedding_size=cfg.mweight_volume.embedding_size,
            volume_size=cfg.mweight_volume.volume_size,
            total_bones=cfg.total_bones)
        self.non_rigid_mlp = _Replicated(_NonRigidParams(
            pos_embed_size=6 * nr.multires, condition_code_size=nr.condition_code_size,
            mlp_width=nr.mlp_width, mlp_depth=nr.mlp_depth, skips=nr.skips))
        # heads of the canonical MLP: 0 = the single-head network, else 2..8 (select_head / forward's head_id)
        self.head_num = canonical_head_num(cfg)
        # bands of the view branch's direction embedding: 0 = colour does not depend on the view (fixed_view / forward)
        self.view_bands = view_dir_bands(cfg)
        self.cnl_mlp = _Replicated(_CanonicalParams(
            input_ch=3 + 6 * cm.multires, mlp_depth=cm.mlp_depth, mlp_width=cm.mlp_width, skips=[4],
            n_heads=max(self.head_num, 1), view_ch=3 + 6 * self.view_bands if self.view_bands else 0))
        if not cfg.get('pose_decoder_off', False):
            self.pose_decoder = BodyPoseRefiner(
                embedding_size=cfg.pose_decoder.embedding_size, mlp_width=cfg.pose_decoder.mlp_width,
                mlp_depth=cfg.pose_decoder.mlp_depth, total_bones=cfg.total_bones)
        # Everything kept from frame to frame is one kept.Kept each, by name: ('pack', head) the packed canonical images
        # (head None = the single-head network, -1 = the all-heads image), 'vol' the decoded weight volume, 'baked' the
        # canonical grid (cfg.amd.canonical = 'baked'), 'baked_nr' the frame's offset grid (cfg.amd.nonrigid = 'baked'),
        # 'head_id' the last device tensor read as a head_id.  weights_changed() drops all that is not injected.
        self._kept = {}
        # the name of the packed image used last (its serial number goes to the f16-range guard), and the packs so far
        self._pack_last = None
        self._pack_serial = 0
        # counts the train-path forwards: compared by every entry's weights test, so that an entry built before one is
        # out of date after it (it stays where it is, its buffers are used again)
        self._weights_gen = 0
        # the head that _canonical_packed() packs outside forward (select_head), None = not chosen
        self._head = None
        # the direction fixed_view chose for colour evaluated without a ray (a tuple of three floats), None = not chosen
        self._view = None
        self._nr_pack_buf = None
        self.f16_guard = InferenceRangeGuard()
        # the bakes this network ran, and the resident workspace of the offset grid's bake
        self.bake_count = 0
        self._nr_bake_ws = None
        self.nonrigid_bake_count = 0
        self._workspace = None
        # the gradient pass's chunk workspace (ops.density_gradient fills it) and the slot table of hnrf_ray_normals
        self._gradient_ws = {}
        self._normals_ws = None
        # cfg.amd.share_underflow: (live counts per chunk on the device, samples) of the last frame, None = path off
        self._share_last = None
        # set by train.Trainer when world_size > 1: dist.GradientSync whose volume_hook averages the weight-volume
        # gradient over the ranks in front of the decoder backward
        self.grad_sync = None
        # set to a list to collect (start, stop) torch.cuda.Event pairs recorded around
        # every canonical-MLP launch (bench.py roofline)
        self.mlp_event_log = None

    # reference API ---------------------------------------------------------
    def deploy_mlps_to_secondary_gpus(self):
        """No-op: every GPU runs the whole renderer (network.py:161-166)."""
        return self

    # packed-weight caches ----------------------------------------------------
    def weights_changed(self):
        """Drop everything derived from the parameters -- the packed canonical images, the decoded weight volume, the
        baked canonical grid (an injected one stays: set_baked_grid) and the frame's offset grid -- and restart the
        f16-range guard's audit schedule: the next frame rebuilds from the parameters as they are then.  THE call after
        any write the entries cannot see by themselves (kept._resident: writes through ``p.data`` / ``p.detach()``, e.g.
        ``p.data.copy_()``, ``dist.broadcast(p.data)``, an optimizer that steps through detached views).
        load_state_dict and every move / cast of the module (``to``, ``cpu``, ``cuda``, ``float``) call it themselves; a
        train-path forward marks the entries out of date to the same effect (_weights_gen).  Host only: no device work,
        no synchronisation."""
        self._drop(lambda e: not e.injected)
        self.f16_guard.restart_schedule()
        return self

    def _drop(self, which):
        for name in [n for n, e in self._kept.items() if which(e)]:
            del self._kept[name]

    def load_state_dict(self, *args, **kwargs):
        try:
            return super().load_state_dict(*args, **kwargs)
        finally:
            self.weights_changed()               # (also after a load that raised half way)

    def _apply(self, fn, *args, **kwargs):
        try:
            return super()._apply(fn, *args, **kwargs)
        finally:
            self.weights_changed()               # (a move frees the old storage: its address may come back)

    def _mlp_mode(self):
        return self.f16_guard.mode()

    # f16-range guard (range_guard.InferenceRangeGuard) ------------------------
    f16_range_hits = property(lambda self: self.f16_guard.hits)
    f16_range_watched = property(lambda self: self.f16_guard.watched)
    f16_range_checked = property(lambda self: self.f16_guard.checked)

    def check_f16_range(self, wait=True, upto=None):
        """Act on the verdicts of the watched frames (InferenceRangeGuard.check, then its policy step ``act``; render
        loops call this once after their last frame).  Returns True when one of them left the range."""
        hit = self.f16_guard.check(wait, upto)
        if any(hit):
            self._drop(lambda e: e.packed is not None)          # (a fresh pack clears the canonical image's word)
        return self.f16_guard.act(*hit)

    def _canonical_pass(self, op, colour=None):
        """``op(packed canonical image, mode)`` of a canonical-MLP pass outside forward (``colour``: _canonical_packed's),
        with its status word acted on
        exactly as forward does (cfg.amd.on_f16_range: raise, warn and switch to 'f32', or ignore): after a hit that
        forced another mode the pass runs again in that mode, so the result returned is one of _mlp_mode().  Waits
        for the device."""
        while True:
            mode, packed = self._mlp_mode(), self._canonical_packed(colour)
            res = op(packed, mode)
            if mode != 'f16x3':
                return res
            self.f16_guard.watch(packed, None, mode)
            if not (self.check_f16_range(wait=True) and self._mlp_mode() != mode):
                return res

    def select_head(self, head):
        """Choose the head (0 <= head < head_num) of a multi-head canonical MLP for everything that evaluates it outside
        forward -- mesh extraction, density grid, bake, vertex colours -- and for a forward without ``head_id``; None
        drops the choice.  The head is packed as an ordinary single-head image from rows 4 head .. 4 head + 3 of
        output_linear.0, so every kernel and feature works on it unchanged."""
        if head is not None:
            if not self.head_num:
                raise ValueError('select_head: the canonical MLP has a single head (canonical_mlp.multihead.enable is off)')
            head = int(head)
            if not 0 <= head < self.head_num:
                raise ValueError('select_head: head %d outside 0..%d' % (head, self.head_num - 1))
        self._head = head
        return self

    def _resolve_head(self, head_id):
        """forward's ``head_id`` as an int: -1 = all heads, None = the selected head.  A tensor on the host is read there;
        one on the device is read back once and remembered by the resident-tensor rule, not once per frame."""
        if head_id is None:
            if self._head is None:
                raise RuntimeError('multi-head canonical MLP (%d heads): pass head_id (0..%d, or -1 for all heads) or call '
                                   'select_head first' % (self.head_num, self.head_num - 1))
            return self._head
        if torch.is_tensor(head_id):
            if head_id.numel() != 1:
                raise ValueError('head_id: a tensor of one element, got shape %s' % (tuple(head_id.shape),))
            if head_id.device.type == 'cpu':
                h = int(head_id.reshape(()).item())
            else:
                # read back once per (object, data_ptr, _version), by identity only.  Injected: the caller's value, nothing
                # derived from the weights, so weights_changed() costs no further read-back
                seen = self._kept.get('head_id')
                if seen is None or not seen.fed_by((head_id,)):
                    seen = self._kept['head_id'] = Kept(inputs=(head_id,), injected=True,
                                                        value=int(head_id.reshape(()).item()))
                h = seen.value
        else:
            h = int(head_id)
        if not -1 <= h < self.head_num:
            raise ValueError('head_id %d outside -1..%d' % (h, self.head_num - 1))
        return h

    def fixed_view(self, direction):
        """Choose the viewing direction (3 numbers, any length; observation space) of a view-dependent canonical MLP for
        everything that evaluates colour without a ray -- mesh and glTF vertex colours, the raster preview, bake_canonical
        called directly -- in the manner of select_head; None drops the choice.  B e(direction) is folded into the colour
        bias of the packed image (a host-side add), so every kernel works on it unchanged.  forward never uses it: there
        every ray brings its own direction."""
        if direction is not None:
            if not self.view_bands:
                raise ValueError('fixed_view: the canonical MLP has no view branch (canonical_mlp.view_dir with '
                                 'cfg.amd.view_dir is off)')
            d = torch.as_tensor(direction, dtype=torch.float64).detach().cpu().reshape(-1)
            if d.numel() != 3 or not bool(torch.isfinite(d).all()):
                raise ValueError('fixed_view: a direction of three finite numbers, got %r' % (direction,))
            direction = tuple(float(x) for x in d)
        self._view = direction
        return self

    def _cnl_params(self, biases=True):
        """The canonical MLP's parameters, trunk first, weights then (``biases``) biases: what every entry derived from
        it is keyed on (the RAW parameters, with the view branch its four layers, never the folded tensors)."""
        cm = self.cnl_mlp.module
        lin = cm.trunk() + (cm.view_layers() if self.view_bands else [cm.output_linear[0]])
        return [l.weight for l in lin] + ([l.bias for l in lin] if biases else [])

    def _view_fold(self):
        """(head weight (4, 256), head bias (4,), B (3, 3 + 6 L), zeros (3,)) of the view branch for inference: folded in
        float64 from the detached layers, rounded to fp32 once, kept until the four layers change."""
        layers = self.cnl_mlp.module.view_layers()
        params = [t for l in layers for t in (l.weight, l.bias)]
        ent = self._kept.get('view_fold')
        if ent is None or not ent.built_from(None, self._weights_gen, params):
            with torch.no_grad():
                hw, hb, B = fold_view_branch(*[(l.weight.detach(), l.bias.detach()) for l in layers], dtype=torch.float64)
                value = (hw.float().contiguous(), hb.float().contiguous(), B.float().contiguous(), hb.new_zeros(3).float())
            ent = self._kept['view_fold'] = Kept(None, self._weights_gen, params, value=value)
        return ent.value

    def _cnl_layers(self, colour=None):
        """(weights, biases) of the nine layers the kernels know, detached: the parameters themselves, or with the view
        branch the trunk and the folded head -- ``colour`` 'fixed': with B e(fixed_view's direction) in its colour bias."""
        cm = self.cnl_mlp.module
        if not self.view_bands:
            lin = cm.linears()
            return [l.weight.detach() for l in lin], [l.bias.detach() for l in lin]
        hw, hb, B, _ = self._view_fold()
        if colour == 'fixed':
            e = view_embedding(torch.tensor(self._view, dtype=torch.float64), self.view_bands)
            hb = hb.clone()
            hb[:3] += (B.double().cpu() @ e).float().to(hb.device)
        lin = cm.trunk()
        return [l.weight.detach() for l in lin] + [hw], [l.bias.detach() for l in lin] + [hb]

    def _canonical_packed(self, colour=None):
        """The packed canonical image: of all rows on the single-head network (no head: None in the key), else of the
        selected head (ops.canonical_pack on its four rows) or with head -1 the all-heads image
        (ops.canonical_heads_pack); one kept image per head, the head in its key.  With a view branch the image is the
        folded one, and ``colour`` says what its colour rows are for: 'fixed' = read as they are (vertex colours, a bake
        outside forward) -- needs fixed_view's direction, none is used silently; 'ray' = a per-ray bias follows in K4
        (forward); None = not read at all (density only).  The last two share one image."""
        h = self._head if self.head_num else None
        if self.head_num and h is None:
            raise RuntimeError('multi-head canonical MLP (%d heads): call select_head(h) before evaluating it outside '
                               'forward (no head is used silently)' % self.head_num)
        view = None
        if self.view_bands and colour == 'fixed':
            if self._view is None:
                raise RuntimeError('view-dependent colour: call fixed_view(direction) before evaluating colour without a '
                                   'ray (no direction is used silently)')
            view = self._view
        ws = self._cnl_params()
        mode, name = self._mlp_mode(), ('pack', h) + ((view,) if self.view_bands else ())
        ent = self._kept.get(name)
        if ent is None or not ent.built_from((mode, h), self._weights_gen, ws):
            W, B = self._cnl_layers(colour)
            buf = None if ent is None else ent.packed                   # (a stale image's buffer is packed into again)
            if h is not None and h < 0:
                packed = ops.canonical_heads_pack(W, B, self.head_num, mode, out=buf)
            else:
                if h is not None:
                    W[8], B[8] = W[8][4 * h:4 * h + 4], B[8][4 * h:4 * h + 4]    # (whole rows: contiguous views)
                packed = ops.canonical_pack(W, B, mode, out=buf)
            self._pack_serial += 1                                      # (every pack takes the next serial)
            ent = self._kept[name] = Kept((mode, h), self._weights_gen, ws, packed=packed, serial=self._pack_serial)
        self._pack_last = name                                          # (_guard_plan: the serial of the image used last)
        return ent.packed

    def _nonrigid_packed(self, cond):
        lin = self.non_rigid_mlp.module.linears()
        self._nr_pack_buf = ops.nonrigid_pack([l.weight.detach() for l in lin], [l.bias.detach() for l in lin],
                                              cond.detach().contiguous(), self._mlp_mode(), out=self._nr_pack_buf)
        return self._nr_pack_buf

    def _weight_volume(self, priors):
        """(B+1,G,G,G) softmax volume; cached across frames in eval mode."""
        params = list(self.mweight_vol_decoder.parameters())
        # consulted and stored only in eval mode, with grad disabled and the option on: otherwise the entry is left alone
        use_cache = (not self.training) and (not torch.is_grad_enabled()) and amd_option('cache_weight_volume', True)
        e = self._kept.get('vol') if use_cache else None
        # The kept priors (a clone) are compared by shape first.  Then the ladder: the same tensor object as last frame (a
        # driver that keeps the priors resident) hits without a comparison, i.e. without a host synchronisation; a fresh
        # tensor is compared by value once (a device round trip) and THIS tensor is remembered, so that the frames that
        # follow hit by identity (a render loop uploads the subject's priors once per loop)
        if e is not None and e.built_from(None, self._weights_gen, params) and e.priors.shape == priors.shape \
                and e.fed_by((priors,), lambda: torch.equal(e.priors, priors)):
            return e.vol
        vol = self.mweight_vol_decoder(motion_weights_priors=priors[None])[0].contiguous()
        if use_cache:
            self._kept['vol'] = Kept(None, self._weights_gen, params, (priors,), priors=priors.clone(), vol=vol)
        return vol

    # forward -------------------------------------------------------------------
    def _refines_pose(self, iter_val):
        return iter_val >= cfg.pose_decoder.get('kick_in_iter', 0) and not cfg.get('pose_decoder_off', False)

    def _conditioning(self, dst_posevec, iter_val, dev, want_device_hann, want_rvec=True, want_hann=True):
        """What a frame's pose vector (fp32 on ``dev``) and ``iter_val`` make of the two motion models: (rvec, cond,
        hann_host, hann_w, nr_inputs_are_zero) -- the pose refiner's axis-angle corrections (23, 3) from its kick-in on
        (network.py:667-688; None before it or without ``want_rvec``), the non-rigid MLP's condition code (zeroed below
        non_rigid_motion_mlp.kick_in_iter, network.py:735-737), the Hann window on the host and, with
        ``want_device_hann``, on the device (both None without ``want_hann``), and whether the MLP is fed zeros at every
        sample.  Nothing is read back from the device."""
        rvec = self.pose_decoder.rvec(dst_posevec[None]) if want_rvec and self._refines_pose(iter_val) else None
        nr_cfg = cfg.non_rigid_motion_mlp
        below = iter_val < nr_cfg.kick_in_iter
        cond = torch.zeros_like(dst_posevec) * dst_posevec if below else dst_posevec
        hann_host = hann_w = None
        if want_hann:
            hann_host = hann_window_weights(iter_val, nr_cfg.multires, nr_cfg.kick_in_iter, nr_cfg.full_band_iter)
            if want_device_hann:
                # through pinned memory: a pageable host-to-device copy waits for everything queued on the stream, i.e.
                # it would synchronise host and GPU once per training step / frame
                hann_w = hann_host.pin_memory().to(dev, non_blocking=True) if dev.type == 'cuda' else hann_host.to(dev)
        return rvec, cond, hann_host, hann_w, want_hann and below and float(hann_host.abs().max()) == 0.0

    def forward(self, rays, dst_Rs, dst_Ts, cnl_gtfms, motion_weights_priors, dst_posevec=None,
                near=None, far=None, iter_val=1e7, cnl_bbox_min_xyz=None, cnl_bbox_scale_xyz=None,
                bgcolor=None, t_rand=None, head_id=None, **kwargs):
        """network.py:647-789.  Extra keyword ``t_rand`` (N,S) injects the
        stratified-sampling uniforms (parity tests); unknown kwargs are ignored
        like the reference's **kwargs.  ``head_id`` (multi-head canonical MLP only; an int or a tensor of one element):
        the head to render, None = the one of select_head, -1 = every head of one trunk pass -- the per-head keys are then
        lists of head_num tensors (network.py:570-601)."""
        if self.head_num:
            # the head holds for everything the frame evaluates (the canonical image, a bake), then the selection returns
            prev, self._head = self._head, self._resolve_head(head_id)
            try:
                return self._forward(rays, dst_Rs, dst_Ts, cnl_gtfms, motion_weights_priors, dst_posevec, near, far, iter_val,
                                     cnl_bbox_min_xyz, cnl_bbox_scale_xyz, bgcolor, t_rand, **kwargs)
            finally:
                self._head = prev
        return self._forward(rays, dst_Rs, dst_Ts, cnl_gtfms, motion_weights_priors, dst_posevec, near, far, iter_val,
                             cnl_bbox_min_xyz, cnl_bbox_scale_xyz, bgcolor, t_rand, **kwargs)

    def _forward(self, rays, dst_Rs, dst_Ts, cnl_gtfms, motion_weights_priors, dst_posevec, near, far, iter_val,
                 cnl_bbox_min_xyz, cnl_bbox_scale_xyz, bgcolor, t_rand, **kwargs):
        train_path = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if train_path:
            # a step follows, by whatever optimizer (torch's fused Adam leaves the version counters alone): the next
            # inference frame rebuilds everything derived from the weights
            self._weights_gen += 1
        all_heads = self.head_num and self._head == -1
        if self.head_num and train_path and not amd_option('train_heads', False):
            raise NotImplementedError('multi-head canonical MLP: inference only (the training kernels have one head; '
                                      'checkpoints come from the reference trainer) -- call forward under torch.no_grad(), '
                                      'or set cfg.amd.train_heads = True to train it')
        if self.f16_guard.pending:
            self.check_f16_range(wait=False)       # the previous frames' f16-range verdicts (may switch the mode, or raise)
        iter_val = float(iter_val)
        dev = dst_Rs.device
        f32 = lambda t: t.to(dtype=torch.float32)
        posevec_arg = dst_posevec                  # (the caller's tensor: the per-frame offset grid is keyed by its identity)
        dst_Rs, dst_Ts, dst_posevec = f32(dst_Rs), f32(dst_Ts), f32(dst_posevec)
        cnl_gtfms, priors = f32(cnl_gtfms), f32(motion_weights_priors)

        ignore_nr = bool(cfg.ignore_non_rigid_motions)
        mode = self._mlp_mode()
        canonical, nonrigid, _ = check_amd_options()      # (ValueError: unknown values, 'baked' offsets without a grid)
        # the offsets come from the frame's offset grid: no per-frame pack and no window upload unless it is (re)baked
        nr_from_grid = nonrigid == 'baked' and not train_path and not ignore_nr
        rvec, cond, hann_host, hann_w, nr_inputs_are_zero = self._conditioning(
            dst_posevec, iter_val, dev, not nr_from_grid, want_hann=not ignore_nr)
        motion_Rs, motion_Ts = motion_basis(dst_Rs, dst_Ts, cnl_gtfms, rvec)   # (Rodrigues + correction: in there)
        vol = self._weight_volume(priors)
        self.motion_weights_vol = vol
        if train_path and self.grad_sync is not None:
            vol = self.grad_sync.volume_hook(vol, priors)
        nr_packed, cnl_packed = None, None
        if not train_path:
            cnl_packed = self._canonical_packed('ray')
            if not ignore_nr and not nr_from_grid:
                nr_packed = self._nonrigid_packed(cond)

        rays_shape = rays[1].shape
        rays_o = f32(rays[0]).reshape(-1, 3).contiguous()
        rays_d = f32(rays[1]).reshape(-1, 3).contiguous()
        N, S = rays_o.shape[0], int(cfg.N_samples)
        if cfg.perturb > 0.:
            if t_rand is None:
                t_rand = torch.rand(N, S, device=dev)                       # network.py:468
            t_rand = f32(t_rand).reshape(N, S).contiguous()
        else:
            t_rand = None
        per_ray = (rays_o, rays_d, f32(near).reshape(-1).contiguous(), f32(far).reshape(-1).contiguous(), t_rand)
        per_frame = (motion_Rs, motion_Ts, vol, f32(cnl_bbox_min_xyz).contiguous(), f32(cnl_bbox_scale_xyz).contiguous(),
                     hann_w)
        bg = f32(bgcolor).contiguous()
        diag = bool(amd_option('diagnostics', True))
        term_eps = float(amd_option('term_eps', 0.0))
        view_bias = view_train = None
        if self.view_bands:
            # view-dependent colour: every sample of a ray shares the ray's direction (network.py:499-507), so the branch
            # leaves three floats per ray, computed once per frame here and added to the raw colour in K4
            camera_only = bool(cfg.canonical_mlp.get('view_dir_camera_only', False))
            if camera_only and len(rays) < 3:
                raise ValueError('canonical_mlp.view_dir_camera_only = True needs the camera directions as the third row '
                                 'of rays (rays_d_camera), got %d rows' % len(rays))
            if term_eps > 0.0 and not train_path:
                raise NotImplementedError('cfg.amd.term_eps > 0 with view-dependent colour (canonical_mlp.view_dir): the '
                                          'slab compositor of early ray termination does not take the per-ray bias')
            view_dirs = f32(rays[2]).reshape(-1, 3).contiguous() if camera_only else rays_d
            if view_dirs.shape[0] != N:
                raise ValueError('rays: %d directions for the view branch, %d rays' % (view_dirs.shape[0], N))
            if train_path:
                # the fold in fp32 under autograd, once per step: torch carries the gradient back to the four layers
                hw, hb, Bv = fold_view_branch(*self.cnl_mlp.module.view_layers())
                view_train = (hw, hb, ViewBias.apply(view_dirs, Bv, hb.new_zeros(3)) if N else None)
            elif N:
                _, _, Bv, zero3 = self._view_fold()
                view_bias = ops.view_bias(view_dirs, Bv, zero3)
        if N == 0:
            # a camera that does not see the subject's bbox (the reference's chunk loop, network.py:330-352, has nothing
            # to concatenate then and raises; a render loop should get its background image): the 11 keys, empty
            zero = sum(p.sum() for p in self.parameters() if p.requires_grad) * 0.0 if train_path else None
            out = {k: torch.zeros((0,) + v, device=dev) + (zero if zero is not None and k in ('rgb', 'alpha', 'depth') else 0.0)
                   for k, v in ops.output_shapes(S, self.total_bones, diag or train_path).items()}
            if all_heads:
                out = self._heads_lists(out)
        elif all_heads and not train_path:
            # every head of one trunk pass: the exact MLP path only
            if canonical == 'baked':
                raise NotImplementedError("head_id = -1 with cfg.amd.canonical = 'baked': a baked grid holds one head "
                                          "(select_head, then bake)")
            if term_eps > 0.0:
                raise NotImplementedError('head_id = -1 with cfg.amd.term_eps > 0: early ray termination follows one '
                                          "head's transmittance")
            if nr_from_grid:
                raise NotImplementedError("head_id = -1 with cfg.amd.nonrigid = 'baked'")
            out = self._forward_frame(per_ray, per_frame, nr_packed, cnl_packed, bg, S, mode, diag, hann_host,
                                      all_heads=True)
        elif train_path:
            # (cfg.amd.train_heads: head h >= 0 trains on the single-head kernels, -1 on the all-heads ones)
            out = self._forward_chunks(per_ray, per_frame, bg, S, mode, diag,
                                       train=(cond, not ignore_nr, nr_inputs_are_zero), view=view_train)
            if all_heads:      # the reference's list shapes, like the inference path's
                out = {k: list(v.unbind(0)) if k in ops.HEAD_KEYS else ([v] * self.head_num if k == 'xyz_on_rays' else v)
                       for k, v in out.items()}
        else:
            baked, baked_nr, nr_baked_on = None, None, None
            if canonical == 'baked':                             # (training ignores the option: _render_rays_train)
                if not diag and term_eps > 0.0:
                    raise NotImplementedError("cfg.amd.term_eps > 0 with cfg.amd.canonical = 'baked': early ray termination "
                                              "has no baked form (hnrf_render_rays_term_fwd runs the canonical MLP)")
                baked = self._baked_for_frame(cnl_bbox_min_xyz, kwargs.get('cnl_bbox_max_xyz'), cnl_bbox_scale_xyz)
                if nr_from_grid:
                    # over the canonical grid's box; nr_baked_on: the image this frame's bake ran on (its status word is
                    # watched by _forward_frame), None when the grid of the last frame still holds
                    baked_nr, nr_baked_on = self._baked_nr_for_frame(posevec_arg, iter_val, hann_host, baked[1], baked[2])
            if diag or term_eps == 0.0:    # (with diagnostics on, term_eps is ignored: early termination has no 11-output form)
                out = self._forward_frame(per_ray, per_frame, nr_packed, cnl_packed, bg, S, mode, diag, hann_host,
                                          baked, baked_nr, nr_baked_on, view_bias=view_bias)
            else:
                out = self._forward_chunks(per_ray, per_frame, bg, S, mode, diag, packs=(nr_packed, cnl_packed),
                                           term_eps=term_eps)
        lead = list(rays_shape[:-1])
        shaped = lambda v: v.reshape(lead + list(v.shape[1:]))
        return {k: [shaped(t) for t in v] if isinstance(v, list) else shaped(v) for k, v in out.items()}

    def _heads_lists(self, out):
        """A single-head output dict in the all-heads form: lists of head_num tensors for the per-head keys."""
        H = self.head_num
        return {k: [v.clone() for _ in range(H)] if k in ops.HEAD_KEYS else ([v] * H if k == 'xyz_on_rays' else v)
                for k, v in out.items()}

    def _guard_plan(self, mode, n_rays):
        last = self._kept.get(self._pack_last)
        return self.f16_guard.plan(mode, -(-n_rays // int(cfg.chunk)), None if last is None else last.serial)

    def _forward_frame(self, per_ray, per_frame, nr_packed, cnl_packed, bg, S, mode, diag, hann_host=None, baked=None,
                       baked_nr=None, nr_baked_on=None, all_heads=False, view_bias=None):
        """Inference, the whole frame in one library call -- chunk loop of network.py:330-352, results straight into
        whole-frame tensors (the reference concatenates per-chunk results: one more pass over 17 KB per ray);
        optionally K1 of the next chunk on a side stream under the MLP kernels of the current one
        (cfg.amd.overlap_warp).  ``all_heads``: every head (hnrf_render_frame_heads_fwd, with the shared evaluation of
        underflowing inputs hnrf_render_frame_heads_shared_fwd) -- the trunks of both MLPs once per chunk, one compositing
        pass per head.  ``view_bias`` (N, 3): view-dependent colour, on every path (hnrf_render_frame_view_fwd)."""
        gmode, guarded = self._guard_plan(mode, per_ray[0].shape[0])
        cull_eps = 0.0 if diag else float(amd_option('cull_eps', 0.0))
        common = dict(diagnostics=diag, cull_eps=cull_eps, workspace=self._workspace,
                      overlap=bool(amd_option('overlap_warp', False)), mlp_event_log=self.mlp_event_log)
        # one evaluation for the samples whose inputs underflow to those of x_skel = 0 (hnrf.h, hnrf_share_compact;
        # its threshold assumes Hann weights <= 1: checked on the host copy, nothing waits for the device)
        share = (bool(amd_option('share_underflow', True)) and mode == 'f16x3' and nr_packed is not None
                 and baked is None and cull_eps == 0.0 and float(hann_host.max()) <= 1.0)
        share_log = [] if share else None
        if all_heads:
            out, self._workspace = ops.render_frame_heads(*per_ray, *per_frame, nr_packed, cnl_packed, bg, S,
                                                          int(cfg.chunk), self.head_num, gmode, share_log=share_log,
                                                          **common)
        else:
            out, self._workspace = ops.render_frame(*per_ray, *per_frame, nr_packed, cnl_packed, bg, S, int(cfg.chunk),
                                                    gmode, baked=baked, baked_nr=baked_nr, share_log=share_log,
                                                    **({} if view_bias is None else {'view_bias': view_bias}), **common)
        self._share_last = share_log[0] if share else None
        if mode == 'f16x3' and guarded != set():
            self.f16_guard.watch(cnl_packed, nr_packed if baked_nr is None else nr_baked_on, mode)
        return out

    def _forward_chunks(self, per_ray, per_frame, bg, S, mode, diag, train=None, packs=None, term_eps=0.0, view=None):
        """Per ray chunk (network.py:333): training (``train`` = (cond, use_nonrigid, nr_inputs_are_zero):
        autograd.RenderRays), or the lean inference path with early ray termination (``packs`` = (nr_packed,
        cnl_packed): hnrf_render_rays_term_fwd, one workspace for every chunk).  ``view`` (training with view-dependent
        colour): (folded head weight, folded head bias, the frame's per-ray bias), the bias cut into the chunks' rows."""
        N, chunk = per_ray[0].shape[0], int(cfg.chunk)
        self._share_last = None
        if train is None:
            _, guarded = self._guard_plan(mode, N)
            cull_eps = float(amd_option('cull_eps', 0.0))
            need = ops.render_term_workspace_bytes(min(chunk, N), S) // 4 + 64
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != per_ray[0].device:
                self._workspace = torch.empty(need, device=per_ray[0].device)
        chunks = []
        for ci, i in enumerate(range(0, N, chunk)):
            part = [None if t is None else t[i:i + chunk] for t in per_ray]
            if train is not None:
                chunks.append(self._render_rays_train(*part, *per_frame, train[0], bg, S, train[1], diag, train[2],
                                                      view=None if view is None else view[:2] + (view[2][i:i + chunk],)))
                continue
            chunks.append(ops.render_rays_term(*part, *per_frame, *packs, bg, S,
                                               mode if guarded is None or ci in guarded else mode + '+noguard',
                                               term_eps=term_eps, cull_eps=cull_eps, workspace=self._workspace))
        if train is None and mode == 'f16x3' and guarded != set():
            self.f16_guard.watch(packs[1], packs[0], mode)
        # (all heads in training: the per-head keys come head-major, [H, rays, ...])
        ray_dim = lambda k: 1 if train is not None and self.head_num and self._head == -1 and k in ops.HEAD_KEYS else 0
        return {k: (torch.cat([c[k] for c in chunks], ray_dim(k)) if len(chunks) > 1 else chunks[0][k]) for k in chunks[0]}

    def shared_sample_share(self):
        """Share of the last frame's samples that took the shared evaluation of cfg.amd.share_underflow instead of a pass
        through the MLPs (0.0 when the path was off for that frame).  Waits for the device: for profiling tools and
        tests, not for render loops."""
        if self._share_last is None:
            return 0.0
        live, total = self._share_last
        torch.cuda.synchronize(live.device)
        return 1.0 - float(live.sum().item()) / float(max(total, 1))

    def _nonrigid_of_zero(self):
        """NonRigidMotionMLP.forward (mlp_offset.py:74-114) on an all-zero input row: (3,), differentiable."""
        lin = self.non_rigid_mlp.module.linears()
        # (through F.linear although W0 @ 0 = 0: W0 must receive its all-zero gradient like in the reference, so that Adam
        # creates its state and counts its steps from the first iteration -- a None gradient would restart the bias
        # correction of W0 at the kick-in iteration)
        h = F.linear(lin[0].weight.new_zeros(lin[0].in_features), lin[0].weight, lin[0].bias)
        for i, l in enumerate(lin[1:-1], start=1):
            h = torch.relu(h)
            if l.in_features != h.shape[0]:                         # the skip layer takes [h | PE36], and the PE is zero too
                h = torch.cat([h, h.new_zeros(l.in_features - h.shape[0])])
            h = F.linear(h, l.weight, l.bias)
        return F.linear(torch.relu(h), lin[-1].weight, lin[-1].bias)

    def _render_rays_train(self, rays_o, rays_d, near, far, t_rand, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale,
                           hann_w, cond, bg, S, use_nonrigid, diag, nr_inputs_are_zero, view=None):
        """Differentiable chunk: autograd.RenderRays (activation-saving MLP kernels).  rgb / alpha / depth carry
        gradient (the trainer's loss reads rgb, trainer.py:121); with ``cfg.amd.diagnostics`` the other eight keys of
        the reference's return dict (network.py:776-789) are returned too, detached.  cfg.amd.canonical = 'baked' is
        ignored here: training always evaluates the canonical MLP (the grid has no gradient)."""
        nr = self.non_rigid_mlp.module.linears()
        if hann_w is None:
            hann_w = torch.ones(6, device=rays_o.device)
        if view is not None:
            # view-dependent colour: the folded head as layer 8 and the chunk's per-ray bias -- no kernel sees the
            # unfolded branch
            cn = self.cnl_mlp.module.trunk()
            cn_w, cn_b = [l.weight for l in cn] + [view[0]], [l.bias for l in cn] + [view[1]]
        else:
            cn = self.cnl_mlp.module.linears()
            cn_w, cn_b = [l.weight for l in cn], [l.bias for l in cn]
        if self.head_num and self._head >= 0:
            # one head of a multi-head MLP (cfg.amd.train_heads): views of its four rows, as select_head packs them --
            # autograd leaves zeros in the other heads' rows, like the reference's slice (mlp_rgb_sigma.py:189-191)
            rows = slice(4 * self._head, 4 * self._head + 4)
            cn_w[8], cn_b[8] = cn_w[8][rows], cn_b[8][rows]
        params = [l.weight for l in nr] + [l.bias for l in nr] + cn_w + cn_b
        const_offset = None
        if use_nonrigid and nr_inputs_are_zero:
            # before non_rigid_motion_mlp.kick_in_iter the MLP is fed zeros at every sample (condition code x 0,
            # network.py:735-737; Hann weights all 0, hannw_fourier.py:28-40): its offset is the per-frame constant MLP(0)
            # (SURVEY section 7).  Evaluated once, in fp32 with torch's autograd, instead of 786 432 times: the first
            # 10 000 (ZJU) / 100 000 (wild) iterations of a run lose the non-rigid kernels' forward, chain and weight
            # gradients (1.9 of 10 ms), and their near-zero activations never meet the f16 operand range.
            const_offset = self._nonrigid_of_zero()
            use_nonrigid = False
        res = RenderRays.apply(rays_o, rays_d, near, far, t_rand, bbox_min, bbox_scale, hann_w,
                               cond.detach().contiguous(), bg, S, use_nonrigid, diag, const_offset, motion_Rs, motion_Ts, vol,
                               *params, *(() if view is None else (view[2],)))
        return dict(zip(RenderRays.OUTPUT_KEYS if diag else RenderRays.OUTPUT_KEYS[:3], res))

    # baked canonical grid (no counterpart in the reference; humannerf_amd/baked.py) --------------------------------
    def _cnl_tensors(self):
        cm = self.cnl_mlp.module
        lin = cm.trunk() + cm.view_layers() if self.view_bands else cm.linears()
        return [t for l in lin for t in (l.weight, l.bias)]

    def _view_key(self, colour):
        """What a baked grid's key says about its colour rows: () without a view branch, else (fixed_view's direction,) or
        (None,) for a grid whose colour waits for the per-ray bias."""
        return ((self._view if colour == 'fixed' else None),) if self.view_bands else ()

    def canonical_weights_hash(self):
        """sha256 of the canonical MLP's weights (baked.weights_hash): what save_grid stores with a grid."""
        from . import baked
        return baked.weights_hash(self._cnl_tensors())

    def bake_canonical(self, cnl_bbox_min_xyz, cnl_bbox_max_xyz=None, resolution=None, cnl_bbox_scale_xyz=None,
                       colour='fixed'):
        """Tabulate the canonical MLP on a resolution^3 lattice (default cfg.amd.bake_resolution) over
        [cnl_bbox_min_xyz, cnl_bbox_max_xyz] (max absent: min + 2 / cnl_bbox_scale_xyz) with hnrf_bake_canonical, in
        the current mlp_mode, with the f16-range re-run of canonical_density_grid.  Returns the grid (N, N, N, 4)
        float16 on the device and caches it for forward (cfg.amd.canonical = 'baked').  Warns when an output left the
        f16 range and was saturated.  One host synchronisation (the verdicts): call it once per checkpoint.  With a view
        branch ``colour`` = 'fixed' bakes fixed_view's direction into the colour (it raises without one); the baked
        renderer bakes with 'ray': the grid stays a pure function of position and K4 adds the per-ray bias."""
        from . import baked as baked_mod
        with torch.no_grad():
            N = baked_mod.check_resolution(amd_option('bake_resolution', 256) if resolution is None else resolution)
            dev = self._mesh_device()
            # copies: the grid keeps the box it was baked over, whatever the caller writes into these tensors afterwards
            # (_vec3 hands an fp32 device tensor back as it is; _baked_for_frame compares the frame's box with the kept one)
            bmin = _vec3(cnl_bbox_min_xyz, dev).clone()
            bmax = _vec3(cnl_bbox_max_xyz, dev).clone() if cnl_bbox_max_xyz is not None \
                else (bmin + 2.0 / _vec3(cnl_bbox_scale_xyz, dev)).contiguous()
            grid, sat = self._canonical_pass(
                lambda packed, mode: ops.bake_canonical(packed, bmin, bmax, N, mode, want_saturated=True), colour)
            n_sat = int(sat)
            if n_sat:
                import warnings
                warnings.warn('bake_canonical: %d canonical-MLP outputs beyond +-65504 were saturated in the f16 grid: '
                              'the baked render differs from the exact one there' % n_sat)
            self.bake_count += 1
            # key: mode, resolution, selected head.  No input objects remembered: the next frame compares its box by value once
            self._kept['baked'] = Kept((self._mlp_mode(), N, self._head) + self._view_key(colour), self._weights_gen,
                                       self._cnl_tensors(),
                                       grid=grid, bmin=bmin, bmax=bmax)
            return grid

    @property
    def baked_resolution(self):
        """The resolution N of the canonical grid kept for forward (baked or injected), None without one."""
        b = self._kept.get('baked')
        return None if b is None else b.grid.shape[0]

    def set_baked_grid(self, grid, bbox_min, bbox_max, weights_hash=None):
        """Use ``grid`` (float16 (N, N, N, 4), array or tensor; baked.load_grid, or any field on the lattice) over
        [bbox_min, bbox_max] where cfg.amd.canonical = 'baked' asks for one.  An injected grid is never re-baked, whatever
        happens to the weights; ``weights_hash`` (the one stored with a saved grid), when given, must be this network's
        canonical_weights_hash().  ``grid`` None drops the cached grid."""
        if grid is None:
            self._kept.pop('baked', None)
            return
        if weights_hash is not None and weights_hash != self.canonical_weights_hash():
            raise ValueError('set_baked_grid: the grid was baked from other canonical weights (hash %s..., this network '
                             '%s...)' % (str(weights_hash)[:12], self.canonical_weights_hash()[:12]))
        from . import baked as baked_mod
        dev = self._mesh_device()
        g = torch.as_tensor(grid)
        N = baked_mod.check_resolution(g.shape[0])
        if tuple(g.shape) != (N, N, N, 4) or g.dtype != torch.float16:
            raise ValueError('set_baked_grid: grid must be float16 (N, N, N, 4), got %s %s' % (g.dtype, tuple(g.shape)))
        # injected: no key, no weights -- weights_changed() leaves it, _baked_for_frame returns it unconditionally
        self._kept['baked'] = Kept(injected=True, grid=g.to(dev).contiguous(), bmin=_vec3(bbox_min, dev).clone(),
                                   bmax=_vec3(bbox_max, dev).clone())

    # baked non-rigid offset field (no counterpart in the reference; humannerf_amd/baked.py) -------------------------
    def _nr_tensors(self):
        lin = self.non_rigid_mlp.module.linears()
        return [t for l in lin for t in (l.weight, l.bias)]

    def bake_nonrigid(self, dst_posevec, iter_val, box, resolution=None):
        """Tabulate this frame's non-rigid offsets -- a function of x_skel alone once ``dst_posevec`` (the condition
        code; zeroed below non_rigid_motion_mlp.kick_in_iter like in forward) and ``iter_val`` (the Hann window) are
        fixed -- on a resolution^3 lattice (default cfg.amd.nonrigid_bake_resolution) over ``box`` = (bbox_min, bbox_max)
        with hnrf_bake_nonrigid, in the current mlp_mode.  Returns the grid (M, M, M, 4) float16, c = (dx, dy, dz, 0), on
        the device and keeps it for forward (cfg.amd.nonrigid = 'baked').  Nothing is read back: no host
        synchronisation (forward calls this once per frame); the f16-range verdict of the packed image travels with
        forward's watch, and offsets beyond +-65504 m are saturated uncounted."""
        return self._bake_nonrigid(dst_posevec, iter_val, box, resolution).grid

    def _bake_nonrigid(self, dst_posevec, iter_val, box, resolution, key=None, watched=None):
        """bake_nonrigid, returning the entry it keeps.  ``key`` / ``watched``: what _baked_nr_for_frame recognises the
        grid by; a direct call has neither, so no frame hits its grid."""
        from . import baked as baked_mod
        with torch.no_grad():
            M = baked_mod.check_resolution(amd_option('nonrigid_bake_resolution', 128) if resolution is None else resolution)
            dev = self._mesh_device()
            bmin, bmax = _vec3(box[0], dev), _vec3(box[1], dev)
            posevec = torch.as_tensor(dst_posevec).to(device=dev, dtype=torch.float32).reshape(-1)
            _, cond, _, hann, _ = self._conditioning(posevec, float(iter_val), dev, True, want_rvec=False)
            packed = self._nonrigid_packed(cond)
            if self._nr_bake_ws is None or self._nr_bake_ws[0] != (M, dev):
                self._nr_bake_ws = ((M, dev), ops.bake_nonrigid_workspace(M, dev))
            grid = ops.bake_nonrigid(packed, hann, bmin, bmax, M, self._mlp_mode(), workspace=self._nr_bake_ws[1])
            self.nonrigid_bake_count += 1
            b = self._kept['baked_nr'] = Kept(key, self._weights_gen, self._nr_tensors(), watched, grid=grid, bmin=bmin,
                                              bmax=bmax, nr_packed=packed)
            return b

    def _baked_nr_for_frame(self, dst_posevec, iter_val, hann_host, bmin, bmax):
        """((off_grid, bmin, bmax), packed image or None) for an inference frame: the grid of the last frame when its
        key -- mlp_mode, M, the host-side Hann weights, whether the condition code is zeroed -- and the non-rigid
        parameters are unchanged and box and ``dst_posevec`` are the same tensor objects at the same ``_version``; else
        a fresh bake (whose packed image is returned for the f16-range watch, and only then).  Identity only: a fresh
        ``dst_posevec`` tensor re-bakes, nothing is compared by value, nothing synchronises."""
        M = int(amd_option('nonrigid_bake_resolution', 128))
        key = (self._mlp_mode(), M, tuple(hann_host.tolist()), iter_val < cfg.non_rigid_motion_mlp.kick_in_iter)
        watched = (dst_posevec, bmin, bmax)
        b = self._kept.get('baked_nr')
        if b is not None and b.built_from(key, self._weights_gen, self._nr_tensors()) and b.fed_by(watched):
            return (b.grid, b.bmin, b.bmax), None
        b = self._bake_nonrigid(dst_posevec, iter_val, (bmin, bmax), M, key, watched)
        return (b.grid, b.bmin, b.bmax), b.nr_packed

    def _baked_for_frame(self, bbox_min, bbox_max, bbox_scale):
        """(grid, bmin, bmax) for an inference frame: the injected grid, unconditionally; else the kept one when its key
        (mode, N, selected head), the canonical weights and the box match; else a fresh bake over the frame's box.  The
        box is compared like the priors of _weight_volume: the same tensor objects as last frame hit without a look at
        their values (a render loop keeps them resident), fresh tensors are compared by value once (a device round trip)
        and remembered."""
        b = self._kept.get('baked')
        if b is None or not b.injected:
            box = (bbox_min, bbox_max if bbox_max is not None else bbox_scale)
            key = (self._mlp_mode(), int(amd_option('bake_resolution', 256)), self._head) + self._view_key('ray')

            def same_box():
                bmin = _vec3(bbox_min, b.bmin.device)
                bmax = _vec3(bbox_max, bmin.device) if bbox_max is not None else bmin + 2.0 / _vec3(bbox_scale, bmin.device)
                return torch.equal(bmin, b.bmin) and torch.equal(bmax, b.bmax)

            if b is None or not (b.built_from(key, self._weights_gen, self._cnl_tensors()) and b.fed_by(box, same_box)):
                self.bake_canonical(bbox_min, bbox_max, key[1], bbox_scale, colour='ray')
                b = self._kept['baked']
                b.remember(box)
        return b.grid, b.bmin, b.bmax

    # mesh extraction (no counterpart in the reference) ------------------------------------------------------------
    # Density at which the canonical surface is cut.  NOT checked on a trained checkpoint (none can be obtained
    # here): a density of 20 per unit length absorbs about a quarter of the light over 1.6 cm, the sample spacing of
    # 128 samples along a 2 m ray.  Pick the level per checkpoint.
    MESH_LEVEL = 20.0

    def _mesh_device(self):
        return next(self.parameters()).device

    def _mesh_bbox(self, cnl_bbox_min_xyz, cnl_bbox_max_xyz, cnl_bbox_scale_xyz=None):
        dev = self._mesh_device()
        bmin, bmax = _vec3(cnl_bbox_min_xyz, dev), _vec3(cnl_bbox_max_xyz, dev)
        # the datasets' cnl_bbox_scale_xyz = 2 / (max - min) in float32 (dataset.Subject._skeleton_entries)
        scale = _vec3(cnl_bbox_scale_xyz, dev) if cnl_bbox_scale_xyz is not None else (2.0 / (bmax - bmin)).contiguous()
        return bmin, bmax, scale

    def canonical_density_grid(self, cnl_bbox_min_xyz, cnl_bbox_max_xyz, motion_weights_priors, resolution=256,
                               cnl_bbox_scale_xyz=None, return_parts=False):
        """The canonical density relu(sigma) * fg on a resolution^3 lattice over [cnl_bbox_min_xyz, cnl_bbox_max_xyz]
        (hnrf_density_grid): (N, N, N) indexed [z][y][x].  fg is the foreground gate rendering applies to alpha -- the
        summed bone weights of the weight volume -- under the identity motion.  ``return_parts``: (density, sigma,
        fg)."""
        with torch.no_grad():
            dev = self._mesh_device()
            bmin, bmax, scale = self._mesh_bbox(cnl_bbox_min_xyz, cnl_bbox_max_xyz, cnl_bbox_scale_xyz)
            vol = self._weight_volume(torch.as_tensor(motion_weights_priors).to(device=dev, dtype=torch.float32))
            return self._canonical_pass(lambda packed, mode: ops.density_grid(
                packed, vol, bmin, bmax, scale, int(resolution), mode, want_parts=return_parts))

    def vertex_colors(self, verts):
        """sigmoid(raw[:3]) of the canonical MLP at the vertices (V, 3) -- the activation of _raw2outputs.  With a view
        branch: seen from fixed_view's direction (it raises without one)."""
        with torch.no_grad():
            verts = verts.to(device=self._mesh_device(), dtype=torch.float32).contiguous()
            if verts.shape[0] == 0:
                return verts.new_zeros(0, 3)
            raw = self._canonical_pass(lambda packed, mode: ops.canonical(verts, packed, mode), 'fixed')
            return torch.sigmoid(raw[:, :3])

    def extract_canonical_mesh(self, cnl_bbox_min_xyz, cnl_bbox_max_xyz, motion_weights_priors, resolution=256,
                               level=MESH_LEVEL, cnl_bbox_scale_xyz=None):
        """The canonical body as a coloured triangle mesh: marching tetrahedra (humannerf_amd.mesh) of
        canonical_density_grid at ``level`` (default MESH_LEVEL, not checked on a trained checkpoint), colours from
        vertex_colors.  Returns verts (V, 3) fp32, faces (F, 3) int32, colors (V, 3) fp32 in [0, 1], on the device.
        The surface is open where it meets the bbox."""
        from . import mesh
        density = self.canonical_density_grid(cnl_bbox_min_xyz, cnl_bbox_max_xyz, motion_weights_priors, resolution,
                                              cnl_bbox_scale_xyz)
        verts, faces = mesh.mesh_from_density(density, cnl_bbox_min_xyz, cnl_bbox_max_xyz, level)
        return verts, faces, self.vertex_colors(verts)

    # density-gradient normals (no counterpart in the reference; include/hnrf_normals.h) --------------------------
    def _bwd_packed(self, which):
        """The backward image (hnrf_*_bwd_pack) of the 'canonical' or the 'nonrigid' MLP that density_gradient's dX chain
        reads: one kept entry per (mode, head), built from the weights as the forward images are, not once per call."""
        mode = self._mlp_mode()
        if which == 'canonical':
            h = self._head if self.head_num else None
            # (with a view branch: the folded head, which like every weight of the chain depends on no bias)
            ws, layers = self._cnl_params(biases=False), lambda: self._cnl_layers()[0]
        else:
            h, lin = None, self.non_rigid_mlp.module.linears()
            ws, layers = [l.weight for l in lin], lambda: [l.weight.detach() for l in lin]
        name = ('pack_bwd', which, h)
        ent = self._kept.get(name)
        if ent is None or not ent.built_from((mode, h), self._weights_gen, ws):
            W = layers()
            if h is not None:
                W[8] = W[8][4 * h:4 * h + 4]
            pack = ops.canonical_bwd_pack if which == 'canonical' else ops.nonrigid_bwd_pack
            ent = self._kept[name] = Kept((mode, h), self._weights_gen, ws,
                                          packed=pack(W, mode, out=None if ent is None else ent.packed))
        return ent.packed

    def _gradient_head(self, what):
        if self.head_num and (self._head is None or self._head < 0):
            raise RuntimeError('multi-head canonical MLP (%d heads): call select_head(h) before %s (the gradient is one '
                               "head's; all heads at once are not built)" % (self.head_num, what))

    def _density_gradient(self, pts, warp=None):
        """ops.density_gradient with this network's images and its one resident workspace.  ``warp``: (x_skel, hann_w,
        nr_packed)."""
        if warp is not None:
            warp = tuple(warp) + (self._bwd_packed('nonrigid'),)
        return ops.density_gradient(pts, self._canonical_packed(), self._bwd_packed('canonical'), self._mlp_mode(),
                                    warp=warp, workspace=self._gradient_ws)

    def density_gradient(self, points, frame=None, iter_val=1e7):
        """The gradient of the density with respect to position at ``points`` (P, 3), by the training kernels
        (ops.density_gradient) in _mlp_mode(): (g (P, 3), sigma (P,)) on the device.  ``points`` are canonical; given
        ``frame`` (a frame dict: dst_posevec) they are skeleton-space points of that frame and the non-rigid chain is
        included: g = (I + J_offset)^T grad sigma at x_skel + offset (with cfg.ignore_non_rigid_motions there is no
        offset).  A multi-head network uses the selected head; head -1 raises."""
        self._gradient_head('density_gradient')
        dev = self._mesh_device()
        with torch.no_grad():
            pts = torch.as_tensor(points).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
            if frame is None or bool(cfg.ignore_non_rigid_motions):
                return self._density_gradient(pts)
            posevec = torch.as_tensor(frame['dst_posevec']).to(device=dev, dtype=torch.float32).reshape(-1)
            _, cond, _, hann_w, _ = self._conditioning(posevec, float(iter_val), dev, True, want_rvec=False)
            return self._density_gradient(None, (pts, hann_w, self._nonrigid_packed(cond)))

    def ray_normals(self, data, out, alpha_min=0.5, weight_min=None, iter_val=1e7, want_parts=False):
        """One observation-space normal per ray of a rendered frame from the gradient of the density (hnrf_ray_normals):
        (normal (N, 3) fp32, nvalid (N,) uint8) on the device.  ``data``: the frame's inputs as forward got them;
        ``out``: what forward returned with cfg.amd.diagnostics (weights_on_rays, backward_motion_weights, xyz_on_rays,
        alpha); ``weight_min`` (default cfg.amd.normal_weight_min): a sample takes part iff its compositing weight is
        >= it.  Defined for cfg.perturb == 0: the samples are then the render's own.

        The steps: hnrf_compact_samples over the weights; x_skel of the kept samples from hnrf_sample_warp_fwd run again
        on the frame's rays, chunk by chunk (xyz_on_rays - offsets is not x_skel in fp32); the gradient pass with the
        non-rigid chain behind it; hnrf_ray_normals.  The chain is skipped -- the gradient is taken at xyz_on_rays --
        with cfg.ignore_non_rigid_motions, and below non_rigid_motion_mlp.kick_in_iter, where forward feeds the MLP
        zeros and the offset is a per-frame constant (unless the offsets came from a baked grid).  The MLPs are always
        evaluated, also with cfg.amd.canonical = 'baked': the normals are the exact field's.

        ONE device count is read back per frame -- the number of kept samples, because the training kernels take their
        sample count from the host: unlike the rest of a frame this call waits for the device.  ``want_parts``: also
        return dict(idx, count, n: the kept samples; x: the points the gradient was taken at, skeleton-space when
        ``chain``; g: the gradients)."""
        self._gradient_head('ray_normals')
        if float(cfg.perturb) > 0.:
            raise ValueError('ray normals are defined for cfg.perturb == 0 only (got %r): the samples of the render are '
                             'not reproduced otherwise' % (cfg.perturb,))
        for k in ('weights_on_rays', 'backward_motion_weights', 'xyz_on_rays'):
            if k not in out:
                raise ValueError('ray_normals needs %r of a frame rendered with cfg.amd.diagnostics = True' % k)
        weight_min = float(amd_option('normal_weight_min', 1e-4) if weight_min is None else weight_min)
        iter_val = float(iter_val)
        f32 = lambda t: torch.as_tensor(t).to(dtype=torch.float32)
        with torch.no_grad():
            S = int(out['weights_on_rays'].shape[-1])
            w = f32(out['weights_on_rays']).reshape(-1, S).contiguous()
            N, dev = w.shape[0], w.device
            bmw = f32(out['backward_motion_weights']).reshape(N, S, -1).contiguous()
            alpha = f32(out['alpha']).reshape(-1).contiguous()
            idx, count = ops.compact_samples(w, weight_min)
            n = int(count.item()) if N else 0                     # THE read-back: the training kernels take P from the host
            kept = idx[:n].long()
            dst_posevec = f32(data['dst_posevec']).to(dev)
            ignore_nr = bool(cfg.ignore_non_rigid_motions)
            rvec, cond, _, hann_w, nr_zero = self._conditioning(dst_posevec, iter_val, dev, True, want_hann=not ignore_nr)
            motion_Rs, motion_Ts = motion_basis(f32(data['dst_Rs']).to(dev), f32(data['dst_Ts']).to(dev),
                                                f32(data['cnl_gtfms']).to(dev), rvec)
            motion_Rs = motion_Rs.contiguous()
            chain = not (ignore_nr or (nr_zero and amd_option('nonrigid', 'mlp') != 'baked'))
            if not chain:
                xs = f32(out['xyz_on_rays']).reshape(-1, 3)[kept].contiguous()
                g, _ = self._density_gradient(xs)
            else:
                vol = self._weight_volume(f32(data['motion_weights_priors']).to(dev))
                rays = data['rays']
                per_ray = (f32(rays[0]).reshape(-1, 3).contiguous(), f32(rays[1]).reshape(-1, 3).contiguous(),
                           f32(data['near']).reshape(-1).contiguous(), f32(data['far']).reshape(-1).contiguous())
                bmin, bscale = f32(data['cnl_bbox_min_xyz']).contiguous(), f32(data['cnl_bbox_scale_xyz']).contiguous()
                xs = torch.zeros(n, 3, device=dev)
                chunk = int(cfg.chunk)
                for r0 in range(0, N, chunk):
                    part = [t[r0:r0 + chunk] for t in per_ray]
                    x_skel = ops.sample_warp(*part, None, motion_Rs, motion_Ts.contiguous(), vol, bmin, bscale, S)[1]
                    local = kept - r0 * S
                    inside = (local >= 0) & (local < x_skel.shape[0] * S)
                    xs = torch.where(inside[:, None], x_skel.reshape(-1, 3)[local.clamp(0, x_skel.shape[0] * S - 1)], xs)
                g, _ = self._density_gradient(None, (xs, hann_w, self._nonrigid_packed(cond)))
            if self._normals_ws is None or self._normals_ws.numel() < N * S or self._normals_ws.device != dev:
                self._normals_ws = torch.empty(max(N * S, 1), dtype=torch.int32, device=dev)
            normal, nvalid = ops.ray_normals(w, bmw, motion_Rs, idx, count, g, alpha, alpha_min, workspace=self._normals_ws)
        if want_parts:
            return normal, nvalid, dict(idx=idx, count=count, n=n, g=g, x=xs, chain=chain)
        return normal, nvalid

    def vertex_normals(self, verts, motion_weights_priors, cnl_bbox_min_xyz, cnl_bbox_max_xyz, cnl_bbox_scale_xyz=None,
                       want_parts=False):
        """Unit normals (V, 3) of the surface extract_canonical_mesh cuts at canonical vertices (V, 3): -grad D / |grad D|
        of the gated density D = relu(sigma) fg of canonical_density_grid (hnrf_field_normals), grad sigma from
        density_gradient and grad fg from the weight volume's trilinear weights.  0 where the gradient vanishes.
        ``want_parts``: (normals, g, sigma, vol)."""
        self._gradient_head('vertex_normals')
        with torch.no_grad():
            dev = self._mesh_device()
            bmin, _, scale = self._mesh_bbox(cnl_bbox_min_xyz, cnl_bbox_max_xyz, cnl_bbox_scale_xyz)
            vol = self._weight_volume(torch.as_tensor(motion_weights_priors).to(device=dev, dtype=torch.float32))
            verts = torch.as_tensor(verts).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
            g, sigma = self._density_gradient(verts)
            normals = ops.field_normals(verts, g, sigma, vol, vol.shape[0] - 1, bmin, scale)   # (the background channel is last)
        return (normals, g, sigma, vol) if want_parts else normals

    def refiner_rvec(self, frame, iter_val=1e7):
        """The pose refiner's axis-angle corrections (23, 3) for a frame dict (dst_posevec), as frame_motion applies them
        (dst_Rs[i] <- dst_Rs[i] Rodrigues(rvec[i - 1])); None when iter_val is below its kick_in_iter or it is off."""
        if not self._refines_pose(float(iter_val)):
            return None
        with torch.no_grad():
            posevec = torch.as_tensor(frame['dst_posevec']).to(device=self._mesh_device(), dtype=torch.float32)
            return self.pose_decoder.rvec(posevec[None])

    def frame_motion(self, frame, iter_val=1e7):
        """The motion basis (B,3,3), (B,3) and weight volume forward computes for a frame dict (dst_Rs, dst_Ts,
        cnl_gtfms, motion_weights_priors, dst_posevec), the pose refiner applied when iter_val >= its kick_in_iter."""
        dev = self._mesh_device()
        t = lambda k: torch.as_tensor(frame[k]).to(device=dev, dtype=torch.float32)
        with torch.no_grad():
            dst_Rs, dst_Ts, cnl_gtfms = t('dst_Rs'), t('dst_Ts'), t('cnl_gtfms')
            motion_Rs, motion_Ts = motion_basis(dst_Rs, dst_Ts, cnl_gtfms, self.refiner_rvec(frame, iter_val))
            vol = self._weight_volume(t('motion_weights_priors'))
        return motion_Rs.contiguous(), motion_Ts.contiguous(), vol

    def pose_vertices(self, verts, frame, iter_val=1e7):
        """Canonical vertices (V, 3) -> the frame's pose by forward linear blend skinning (hnrf_forward_skin):
        x_o = sum_b w_b(x_c) A_b^-1(x_c) / max(sum_b w_b, 1e-4) with the frame's motion basis A_b and the bone weights
        of the weight volume at the canonical vertex -- the counterpart of the inverse warp rendering applies.  The
        non-rigid offsets are not inverted: the posed mesh is the skinned canonical surface.  ``frame``: a
        dataset.Subject.movement_frame dict (or any dict with forward's per-frame inputs)."""
        motion_Rs, motion_Ts, vol = self.frame_motion(frame, iter_val)
        dev = self._mesh_device()
        bmin, scale = _vec3(frame['cnl_bbox_min_xyz'], dev), _vec3(frame['cnl_bbox_scale_xyz'], dev)
        with torch.no_grad():
            verts = verts.to(device=self._mesh_device(), dtype=torch.float32).contiguous()
            return ops.forward_skin(verts, motion_Rs, motion_Ts, vol, bmin, scale)

    def skin_weights(self, verts, frame=None, k=4, motion_weights_priors=None, cnl_bbox_min_xyz=None,
                     cnl_bbox_scale_xyz=None):
        """The bone weights pose_vertices blends canonical vertices (V, 3) with, as data (hnrf_skin_weights): the k
        (4 or 8) largest per vertex of the weight volume forward uses, normalised -- what a skinned mesh file holds.
        ``frame``: a frame dict (motion_weights_priors, cnl_bbox_min_xyz, cnl_bbox_scale_xyz; the weights do not depend
        on the pose), or give the three by keyword.  Returns (joints (V, k) uint8, weights (V, k) fp32, kept (V,) fp32
        = the sum of the k selected weights before normalisation) on the device."""
        from . import skin
        frame = frame or {}
        pick = lambda given, key: frame[key] if given is None else given
        dev = self._mesh_device()
        bmin = _vec3(pick(cnl_bbox_min_xyz, 'cnl_bbox_min_xyz'), dev)
        scale = _vec3(pick(cnl_bbox_scale_xyz, 'cnl_bbox_scale_xyz'), dev)
        with torch.no_grad():
            priors = torch.as_tensor(pick(motion_weights_priors, 'motion_weights_priors'))
            vol = self._weight_volume(priors.to(device=dev, dtype=torch.float32))
            verts = verts.to(device=dev, dtype=torch.float32).contiguous()
            return skin.skin_weights(verts, vol, bmin, scale, k=k)

    def render_mesh(self, verts, faces, colors, frame, iter_val=1e7, posed=False, **raster_options):
        """A picture of the mesh in a frame's pose and camera (humannerf_amd.raster, hnrf_raster_mesh): the canonical
        vertices are posed with pose_vertices unless ``posed``; ``K``, ``E``, ``img_height``, ``img_width`` and
        ``bgcolor`` (0..255 in frame dicts) come from the frame -- a camera frame (dataset.Subject frames,
        scene.synthetic_frame(camera_only=True)); host-ray frames carry no camera.  ``raster_options``: cull, shade,
        z_near.  Returns dict(rgb (H, W, 3), alpha, depth (H, W), tri_id (H, W) int32) on the device."""
        import numpy as np
        from . import raster
        from ._lib import HnrfError
        for k in ('K', 'E', 'img_height', 'img_width', 'bgcolor'):
            if k not in frame:
                raise HnrfError('render_mesh: the frame has no %r (a camera frame is needed, not a host-ray frame)' % k)
        dev = self._mesh_device()
        verts = verts.to(device=dev, dtype=torch.float32).contiguous()
        if not posed:
            verts = self.pose_vertices(verts, frame, iter_val)
        host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else a
        bg = np.asarray(host(frame['bgcolor']), dtype=np.float32).reshape(3) / np.float32(255.)
        return raster.rasterize(verts, faces, colors, host(frame['K']), host(frame['E']), int(frame['img_height']),
                                int(frame['img_width']), bgcolor=bg, **raster_options)
