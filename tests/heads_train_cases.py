"""Shared by the multi-head training tests: problems for the all-heads training kernels (a canonical MLP whose
output_linear.0 is (4H, 256), positions, one incoming gradient plane per head) on the problem maker and the fp64
references of tests/test_train_kernel_refs.py, which serve a head layer of any width unchanged."""
import numpy as np

from tests.multihead_cases import head_tensors
from tests.test_train_kernel_refs import make_problem

# 2: one (q, half) pair; 3: an empty half; 5: past the split-f16 k-step boundary (4 H > 16); 8: the full tile
HEAD_COUNTS = [2, 3, 5, 8]


def make_heads_problem(H, P, seed, tiny_head=None):
    """make_problem('canonical', ...) with the head tensors of ``H`` heads (multihead_cases.head_tensors, un-scaled sigma)
    and pr['g'] (H, P, 4): the planes of the incoming gradient, ~30 % of the samples without any (as make_problem has
    them).  ``tiny_head``: that head's rows are uniform in +-1e-5 (the reference's initialisation of small last layers),
    next to normal ones."""
    pr = make_problem('canonical', P, seed)
    rs = np.random.RandomState(seed + 17 * H)
    W, b = head_tensors(H, seed=seed, sigma_scale=1.0)
    if tiny_head is not None:
        W[4 * tiny_head:4 * tiny_head + 4] = rs.uniform(-1e-5, 1e-5, (4, 256)).astype(np.float32)
        b[4 * tiny_head:4 * tiny_head + 4] = rs.uniform(-1e-5, 1e-5, 4).astype(np.float32)
    keep = rs.uniform(size=(1, P, 1)) > 0.3
    g = (rs.standard_normal((H, P, 4)) * keep).astype(np.float32)
    return dict(pr, H=H, ws=pr['ws'][:-1] + [W], bs=pr['bs'][:-1] + [b], g=g)


def head_problem(pr, h, g=None):
    """The single-head problem of head ``h``: rows 4h .. 4h+3 of the head layer, plane h of the gradient."""
    g = pr['g'] if g is None else g
    return dict(pr, ws=pr['ws'][:-1] + [pr['ws'][-1][4 * h:4 * h + 4]], bs=pr['bs'][:-1] + [pr['bs'][-1][4 * h:4 * h + 4]],
                g=np.ascontiguousarray(g[h]))


def wide_gradient(g):
    """(H, P, 4) planes -> the (P, 4H) gradient at the output of the (4H, 256) head layer."""
    return np.ascontiguousarray(np.transpose(g, (1, 0, 2)).reshape(g.shape[1], -1))


# ---- the end-to-end gradient case (tests/make_golden_multihead_train.py, tests/test_gpu_heads_train.py): the scene of
# grad_s64 (tests/golden/meta.json) with three heads whose sigma is scaled to its 64 samples per ray
TRAIN_HEADS = 3
TRAIN_SIGMA_SCALE = 64 / 128.0
# Seed of the per-head loss weights.  The scene has discrete decisions (a ReLU, a voxel cell) that an fp32 evaluation
# takes differently from fp64, and how far that moves a gradient depends on the loss weights: with some sets the three
# heads' terms cancel on a small tensor and ANY fp32 evaluation, the reference's included, is 1e-2 in norm / 3e-4 in
# 1 - cosine from fp64 there.  The end-to-end bounds (6e-3 / 0.99998) were set against a reference that is within 4.4e-3 /
# 1e-5 of fp64 (tests/test_grad_oracle.py::test_reference_gradient_noise_floor), so the case must be one where it is:
# 116 is the first seed from 110 upwards for which the oracle evaluated in fp32 is within 4.4e-3 and 1e-5 of its fp64 run
# for both fixtures (head 1 alone, all heads) -- the code under test has no part in the choice -- and the generator
# records the reference's own distance with the fixtures (110 .. 115 give 1 - cosine between 3.6e-6 and 2.9e-4).
LOSS_SEED = 116


def train_state(base_state):
    """``base_state`` (seeded.seeded_state of the default shapes) with the three training heads."""
    from tests.multihead_cases import B_KEY, W_KEY
    st = dict(base_state)
    st[W_KEY], st[B_KEY] = head_tensors(TRAIN_HEADS, sigma_scale=TRAIN_SIGMA_SCALE)
    return st


def head_loss_weights(n_rays):
    """(H, n_rays, 5): grad_s64's loss weights (columns rgb, alpha, depth), one seeded set per head."""
    return np.stack([np.random.RandomState(LOSS_SEED + h).randn(n_rays, 5).astype(np.float32) for h in range(TRAIN_HEADS)])
