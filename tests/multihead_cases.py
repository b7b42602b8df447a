"""Shared by the multi-head tests and tests/make_golden_multihead.py: the seeded head tensors, and the fp64 twin of the
multi-head canonical MLP (head_depth 1) -- the head layer and the per-head compositing -- stated with the CPU oracle on
a state whose output_linear.0 holds only the head's four rows (mlp_rgb_sigma.py:189-191: outputs[..., 4h:4h+4])."""
import math

import numpy as np
import torch

from oracle import oracle

W_KEY, B_KEY = 'cnl_mlp.module.output_linear.0.weight', 'cnl_mlp.module.output_linear.0.bias'
HEAD_SEED = 20
FIXTURE_HEADS = (3, 8)
# the scene of the fixture: the default golden frame (tests/golden/meta.json 'frame', ~260 rays) at S = 16, iter 1e7
FIXTURE_S = 16


# The golden cases' per-ray tolerances (rgb, alpha 2e-5 on the GPU, 1e-5 for the fp32 oracle) were measured on the seeded
# head at S = 128 samples per ray.  At S = 16 the samples are 8 times as far apart, so the same sigma would give 8 times
# the optical depth per sample -- the regime of the 'dense' golden cases, whose rays saturate and whose per-ray noise is
# larger.  The fixture stays a NON-dense case: sigma (its row's gain and its bias) is scaled by S / 128, which keeps the
# optical depth per sample of the eval_s128 case.
SIGMA_SCALE = FIXTURE_S / 128.0


def head_tensors(n_heads, seed=HEAD_SEED, sigma_scale=SIGMA_SCALE):
    """(4H, 256) weight and (4H,) bias of a multi-head output_linear.0, every head scaled like the single head of
    humannerf_amd.seeded (logits x 3, the sigma row x SIGMA_GAIN and its bias + SIGMA_BIAS) from a stream of its own,
    sigma then x ``sigma_scale`` (above)."""
    from humannerf_amd.seeded import SIGMA_BIAS, SIGMA_GAIN
    rs = np.random.RandomState(seed + n_heads)
    b = math.sqrt(2.0) * math.sqrt(6.0 / (4 + 256))
    W = rs.uniform(-b, b, size=(4 * n_heads, 256)) * 3.0
    bias = rs.uniform(-0.05, 0.05, size=(4 * n_heads,))
    W[3::4] *= SIGMA_GAIN * sigma_scale
    bias[3::4] = (bias[3::4] + SIGMA_BIAS) * sigma_scale
    return W.astype(np.float32), bias.astype(np.float32)


def multihead_state(base_state, n_heads, seed=HEAD_SEED):
    """``base_state`` (seeded.seeded_state of the default shapes) with the head tensors of ``n_heads`` heads."""
    st = dict(base_state)
    st[W_KEY], st[B_KEY] = head_tensors(n_heads, seed)
    return st


def head_state(state, h):
    """The single-head state of head ``h``: rows 4h .. 4h+3 of output_linear.0, everything else shared."""
    st = dict(state)
    st[W_KEY], st[B_KEY] = state[W_KEY][4 * h:4 * h + 4], state[B_KEY][4 * h:4 * h + 4]
    return st


def n_heads_of(state):
    return state[W_KEY].shape[0] // 4


def _t64(state, prefix='cnl_mlp'):
    return {k: torch.as_tensor(np.asarray(v)).double() for k, v in state.items() if k.startswith(prefix)}


def heads_raw64(state, pe=None, xyz=None):
    """fp64 raw of every head, a list of (P, 4): the trunk once, the head layer's rows split by head.  ``pe`` (P, 63), or
    ``xyz`` (P, 3) to encode."""
    st = _t64(state)
    if pe is None:
        pe = oracle.fourier_pe(torch.as_tensor(xyz).double(), 10)
    out = oracle.canonical_mlp(st, torch.as_tensor(pe).double())
    return [out[:, 4 * h:4 * h + 4].numpy() for h in range(n_heads_of(state))]


def head_raw64(state, h, pe):
    """fp64 raw of head ``h`` alone: the oracle on the state sliced to that head."""
    return oracle.canonical_mlp(_t64(head_state(state, h)), torch.as_tensor(pe).double()).numpy()


def composite_heads64(raws, mask, z, rays_d, xyz, bgcolor):
    """Per-head compositing (network.py:570-587): oracle.raw2outputs once per head.  raws: list of (R, S, 4)."""
    t = lambda a: torch.as_tensor(np.asarray(a)).double()
    return [{k: v.numpy() for k, v in oracle.raw2outputs(t(r), t(mask), t(z), t(rays_d), t(xyz), t(bgcolor)).items()}
            for r in raws]


def render_heads(state, frame, S, dtype=torch.float64, heads=None):
    """The frame of every head (a list of the oracle's output dicts): oracle.render on each head's sliced state."""
    heads = range(n_heads_of(state)) if heads is None else heads
    return [{k: v.numpy() for k, v in oracle.render(head_state(state, h), frame, iter_val=1e7, dtype=dtype,
                                                    N_samples=S).items()} for h in heads]
