"""cfg.amd.share_underflow without a GPU: the numpy float32 twin of the predicate (humannerf_amd/shared_input.py, stated
in include/hnrf.h at hnrf_share_compact), the arithmetic facts its threshold rests on, and the choice of the frame that
tests/test_gpu_shared_input.py renders end to end."""
import os
import re

import numpy as np
import pytest

from humannerf_amd import shared_input as si

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = si.SHARE_T
F = np.float32

# the end-to-end frame of tests/test_gpu_shared_input.py: 576 rays x 128 samples, chunks of 128 rays (4 whole + 64)
E2E_FRAME = dict(H=24, W=24)
E2E_SAMPLES, E2E_CHUNK = 128, 128


def crafted_problem():
    """(x [P,3], list of (c_off, c_xyz)): every value class of the predicate on every axis; P = 19 whole
    256-sample blocks of the kernel and a ragged one."""
    above = np.nextafter(T, F(1))
    vals = np.array([0.0, -0.0, 1e-45, -1e-45, 2.0 ** -40, -2.0 ** -40, T, -T, np.nextafter(T, F(0)), above, -above,
                     2.0 ** -20, 1e-3, -1.0, np.nan, np.inf, -np.inf], dtype=F)
    rs = np.random.RandomState(7)
    x = vals[rs.randint(0, 8, size=(4873, 3))]                     # mostly at or under T ...
    hot = rs.rand(4873, 3) < 0.15
    x[hot] = vals[rs.randint(8, len(vals), size=int(hot.sum()))]  # ... some axes of some rows above, NaN or infinite
    x[:len(vals)] = vals[:, None]                                 # every value on all three axes at once
    cs = [np.array([-0.0686608, -0.00916304, 0.06966332], F),     # an offset of the seeded network's size
          np.array([1e-6, -1e-6, 1.5e-6], F),                     # (b) fails where (a) holds, down to ulp(1e-6) / 2
          np.array([0.0, -0.0, 3e-2], F)]                         # exact zeros of both signs
    return x, [(c, (np.zeros(3, F) + c).astype(F)) for c in cs]


def test_threshold_is_the_headers():
    with open(os.path.join(ROOT, 'include', 'hnrf.h')) as f:
        m = re.search(r'#define\s+HNRF_SHARE_T\s+([0-9.eE+-]+)f', f.read())
    assert m and F(float(m.group(1))) == T == F(2.0 ** -31)


def test_what_the_threshold_rests_on():
    """Hann weight <= 1 and |x| <= T: the top octave's PE value is at most 32 T = 2^-26, a factor 2 under the tie 2^-25
    that f16 still rounds to zero; the low part f16(v - 0) is the same conversion."""
    top = F(32.0) * T
    assert top == F(2.0 ** -26)
    assert np.float16(top) == 0 and np.float16(-top) == 0 and np.signbit(np.float16(-top))
    assert np.float16(F(2.0 ** -25)) == 0                          # the tie itself goes to even = 0
    assert np.float16(np.nextafter(F(2.0 ** -25), F(1))) > 0       # and nothing above it does


def test_twin_on_single_values():
    c = np.array([-0.07, -0.009, 0.07], F)
    cx = (np.zeros(3, F) + c).astype(F)
    one = lambda v: bool(si.shared_mask(np.full(3, v, F), c, cx))
    for v in (0.0, -0.0, 1e-45, -1e-45, 2.0 ** -40, -2.0 ** -40, T, -T):
        assert one(v), v
    for v in (np.nextafter(T, F(1)), -np.nextafter(T, F(1)), 2.0 ** -20, 1.0, np.nan, np.inf, -np.inf):
        assert not one(v), v
    # all three axes must pass
    for a in range(3):
        x = np.zeros(3, F)
        x[a] = 2.0 ** -20
        assert not si.shared_mask(x, c, cx)


def test_twin_condition_b():
    """c ~ 1e-6 (ulp 1.1e-13): T and 2^-40 move the sum, 1e-45 does not.  c = +0: only a zero of either sign keeps the
    sum's bits; c = -0: c_xyz is +0 + -0 = +0, which x = -0 does not reproduce."""
    c = np.array([1e-6, -1e-6, 1.5e-6], F)
    cx = (np.zeros(3, F) + c).astype(F)
    one = lambda v, c=c, cx=cx: bool(si.shared_mask(np.full(3, v, F), c, cx))
    assert one(0.0) and one(-0.0) and one(1e-45) and one(-1e-45)
    assert not one(T) and not one(-T) and not one(2.0 ** -40)
    z = np.zeros(3, F)
    assert one(0.0, z, z) and one(-0.0, z, z) and not one(1e-45, z, z) and not one(T, z, z)
    nz = -z
    assert np.signbit(nz).all() and not np.signbit((z + nz).astype(F)).any()
    assert one(0.0, nz, (z + nz).astype(F)) and not one(-0.0, nz, (z + nz).astype(F))


def test_twin_shapes_and_live_list():
    x, cs = crafted_problem()
    for c, cx in cs:
        m = si.shared_mask(x, c, cx)
        assert m.shape == (x.shape[0],) and m.dtype == bool
        assert 0 < m.sum() < m.size
        assert np.array_equal(si.shared_mask(x.reshape(11, 443, 3), c, cx).reshape(-1), m)
        live = si.live_indices(x, c, cx)
        assert np.array_equal(live, np.flatnonzero(~m))
        assert not m[~np.isfinite(x).all(1)].any()                # NaN / inf rows are always live


@pytest.fixture(scope='module')
def e2e_oracle(seeded_params):
    from humannerf_amd import scene
    from oracle import oracle
    fr = scene.synthetic_frame(**E2E_FRAME)
    return oracle.render(seeded_params, fr, iter_val=1e7, N_samples=E2E_SAMPLES)


def test_e2e_frame_has_both_classes(e2e_oracle):
    """The camera of the end-to-end GPU test: between 5 % and 95 % of its samples are shared, judged by the twin on the
    fp32 oracle's x_skel with the oracle's offset at an exactly-zero x_skel as the representative's."""
    x = e2e_oracle['_x_skel'].numpy().reshape(-1, 3)
    off = e2e_oracle['offsets'].numpy().reshape(-1, 3)
    assert x.shape[0] == 576 * E2E_SAMPLES and x.shape[0] // E2E_SAMPLES % E2E_CHUNK != 0
    zero = np.flatnonzero(np.abs(x).max(1) == 0)
    assert zero.size > 0
    c = off[zero[0]]
    share = float(si.shared_mask(x, c, (np.zeros(3, F) + c).astype(F)).mean())
    print('shared share of the end-to-end frame (CPU oracle): %.4f' % share)
    assert 0.05 < share < 0.95
