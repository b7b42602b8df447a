"""The cases of tests/test_gpu_shared_fused.py, chosen and checked without a GPU: K1 with the classification fused in
(hnrf_sample_warp_share_fwd) is compared with K1 + hnrf_share_compact on windows of rays of the end-to-end frame of
tests/test_shared_input_cpu.py, and a window on which every sample falls into one class would not notice a wrong
predicate.  Here the numpy twin of the predicate classifies the fp32 oracle's x_skel of every window and finds both
classes wherever the case says so.

K1 works on R rays of S samples, so a sample count P is R x S with S >= 2: P = 255 / 256 / 257 / 24*128 + 1 are
85 x 3, 2 x 128, 1 x 257 and 7 x 439 (one block short of a sample, one whole, one and a sample, twelve and a sample),
the smallest launch is 1 x 2, and the whole frame (576 x 128: 288 blocks, every chunk shape of the renderer) is the
case whose share of shared samples is known (0.42)."""
import numpy as np
import pytest

from humannerf_amd import shared_input as si
from tests import test_shared_input_cpu as cpu

F = np.float32

# name -> (first ray, rays, samples per ray, both classes present).  The windows start at the image's first ray: about
# 40 % of the samples of the top-left rays are far from every bone (the rays through the image centre stay in the
# body's neighbourhood from near to far: every sample live, which a first choice of windows ran into).
CASES = {
    'P2': (0, 1, 2, False),
    'P255': (0, 85, 3, True),
    'P256': (0, 2, 128, True),
    'P257': (0, 1, 257, True),
    'P3073': (0, 7, 439, True),
    'frame': (0, 576, 128, True),
}


def window(fr, r0, R):
    """The frame dict restricted to rays r0 .. r0 + R - 1."""
    out = dict(fr)
    out['rays'] = np.ascontiguousarray(fr['rays'][:, r0:r0 + R])
    out['near'] = np.ascontiguousarray(fr['near'][r0:r0 + R])
    out['far'] = np.ascontiguousarray(fr['far'][r0:r0 + R])
    return out


@pytest.fixture(scope='module')
def e2e_frame():
    from humannerf_amd import scene
    return scene.synthetic_frame(**cpu.E2E_FRAME)


@pytest.fixture(scope='module')
def representative(seeded_params, e2e_frame):
    """c_off as the oracle has it: the offset of a sample whose x_skel is exactly zero."""
    from oracle import oracle
    out = oracle.render(seeded_params, e2e_frame, iter_val=1e7, N_samples=cpu.E2E_SAMPLES)
    x = out['_x_skel'].numpy().reshape(-1, 3)
    zero = np.flatnonzero(np.abs(x).max(1) == 0)
    assert zero.size > 0
    c = out['offsets'].numpy().reshape(-1, 3)[zero[0]].astype(F)
    return c, (np.zeros(3, F) + c).astype(F), x


@pytest.mark.parametrize('case', sorted(CASES))
def test_case_has_the_classes_it_claims(seeded_params, e2e_frame, representative, case):
    from oracle import oracle
    r0, R, S, both = CASES[case]
    c, cx, x_frame = representative
    assert r0 + R <= e2e_frame['rays'].shape[1] == 576
    if case == 'frame':
        x = x_frame
    else:
        out = oracle.render(seeded_params, window(e2e_frame, r0, R), iter_val=1e7, N_samples=S)
        x = out['_x_skel'].numpy().reshape(-1, 3)
    assert x.shape[0] == R * S
    m = si.shared_mask(x, c, cx)
    print('%s: P = %d, shared %d, live %d' % (case, m.size, int(m.sum()), int((~m).sum())))
    if both:
        assert m.any() and (~m).any()
        # both classes inside one 256-sample block and inside one wave somewhere: the ballot and the block's running
        # offsets are exercised, not only whole blocks of one kind
        P = m.size
        mixed = [0 < m[b:b + 64].sum() < min(64, P - b) for b in range(0, P, 64)]
        assert any(mixed)
    if case == 'frame':
        assert abs(float(m.mean()) - 0.42) < 0.02
        # whole blocks of shared samples between blocks that list some: a block that appends nothing (and issues no
        # atomic) must leave the runs of its neighbours alone, and this window shows it
        live = [int((~m[b:b + 256]).sum()) for b in range(0, m.size, 256)]
        assert any(n == 0 and any(live[:i]) and any(live[i + 1:]) for i, n in enumerate(live))
