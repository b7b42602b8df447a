"""The f16-range guard of the 'f16x3' inference kernels and the accuracy envelope below it.  Needs an MI355X.

'f16x3' splits every operand v into hi = f16(v) and lo = f16(v - hi); the epilogues clamp post-ReLU activations at
65504 and the guarded kernel instances raise HNRF_STATUS_F16_RANGE in the packed image's status word when a finished
activation fragment reaches SAT_HALF (hnrf_mlp_f16.hip, hnrf.h).  The contract: no hit -> the output matches fp32.

Activations are PLANTED: feature j of hidden layer l gets a zero weight row and the bias ``value`` (or a weight on one
PE column, so that only chosen samples get there), and its outgoing column is either zeroed -- only the guard can see
the plant -- or CARRIED, set to c / value, so that the activation takes part in the output at a normal size.  The
expected verdict always comes from the fp64 activations of the oracle, not from the planted number.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_parity import _mlp_states, dev

pytestmark = pytest.mark.gpu

THRESH = 128.0              # the activation at which the guard reports (f16(SAT_HALF), hnrf_mlp_f16.hip)
BAND = 2e-3                 # no case within +-0.2 % of THRESH: there the f16 rounding of hi decides
GATE = 10.0                 # what a position-selective layer-0 feature reaches at the hot samples (below THRESH)

CNL = 'cnl_mlp.module.pts_linears.'
NR = 'non_rigid_mlp.module.block_mlps.'
CNL_HEAD = 'cnl_mlp.module.output_linear.0'
N_HIDDEN = {'cnl': 8, 'nr': 6}
CNL_SKIP, NR_SKIP = 5, 4    # hidden layer whose input holds the PE again: pts_linears.10 [pe, h], block_mlps.8 [h, pe]


def _layer(mlp, l):
    return (CNL if mlp == 'cnl' else NR) + str(2 * l)


def _next_col(mlp, l, j):
    """(name of the layer that reads hidden feature j of layer l, its column)."""
    if mlp == 'cnl':
        if l == 7:
            return CNL_HEAD, j
        return CNL + str(2 * l + 2), (63 + j if l + 1 == CNL_SKIP else j)
    if l == 5:
        return NR + '12', j
    return NR + str(2 * l + 2), j


def _in_col(mlp, k, j):
    """Column of hidden layer k's input that holds hidden feature j of layer k - 1."""
    return 63 + j if (mlp == 'cnl' and k == CNL_SKIP) else j


def plant(st, mlp, l, j, bias, carry=None, gate=None):
    """Feature j of hidden layer l: zero weight row and ``bias``; outgoing column zero (``carry`` None) or ``carry``
    everywhere.  ``gate`` = (PE column, slope, offset): position-selective instead -- layer-0 feature j becomes
    relu(slope * pe + offset) (GATE at the hot samples, 0 elsewhere), layers 1 .. l - 1 pass it on with gain 1 and
    layer l with gain bias / GATE (weights well inside the f16 range), so that only layer l holds the hot value.
    Returns a modified copy of ``st``."""
    st = {k: v.copy() for k, v in st.items()}
    name = _layer(mlp, l)
    st[name + '.weight'][j, :] = 0.0
    st[name + '.bias'][j] = np.float32(bias)
    if gate is not None:
        assert l >= 1
        col, slope, offset = gate
        st[_layer(mlp, 0) + '.weight'][j, :] = 0.0
        st[_layer(mlp, 0) + '.weight'][j, col] = np.float32(slope)
        st[_layer(mlp, 0) + '.bias'][j] = np.float32(offset)
        for k in range(1, l + 1):
            st[_layer(mlp, k) + '.weight'][j, :] = 0.0
            st[_layer(mlp, k) + '.weight'][j, _in_col(mlp, k, j)] = np.float32(1.0 if k < l else bias / GATE)
            st[_layer(mlp, k) + '.bias'][j] = 0.0
    nxt, col = _next_col(mlp, l, j)
    st[nxt + '.weight'][:, col] = 0.0 if carry is None else np.float32(carry)
    return st


def cnl_lists(st):
    names = [CNL + str(i) for i in range(0, 16, 2)] + [CNL_HEAD]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return [T(st[n + '.weight']) for n in names], [T(st[n + '.bias']) for n in names]


def nr_lists(st):
    names = [NR + str(i) for i in range(0, 14, 2)]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return [T(st[n + '.weight']) for n in names], [T(st[n + '.bias']) for n in names]


def oracle_cnl(st, xyz, dtype=torch.float64):
    """(raw, max hidden activation) of the canonical MLP."""
    from oracle import oracle
    s = {k: torch.from_numpy(v).to(dtype) for k, v in st.items() if k.startswith('cnl_mlp')}
    hidden = []
    raw = oracle.canonical_mlp(s, oracle.fourier_pe(torch.from_numpy(xyz).to(dtype), 10), hidden=hidden)
    return raw.numpy(), max(float(h.max()) for h in hidden)


def oracle_nr(st, x, cond, hw, dtype=torch.float64):
    """(offsets, max hidden activation) of the non-rigid MLP."""
    from oracle import oracle
    s = {k: torch.from_numpy(v).to(dtype) for k, v in st.items() if k.startswith('non_rigid_mlp')}
    xt = torch.from_numpy(x).to(dtype)
    hidden = []
    _, ofs = oracle.non_rigid_mlp(s, oracle.hann_pe(xt, hw.to(dtype)), torch.from_numpy(cond).to(dtype)[None], xt,
                                  hidden=hidden)
    return ofs.numpy(), max(float(h.max()) for h in hidden)


def expect_hit(amax):
    assert abs(amax / THRESH - 1.0) > BAND, ('case inside the rounding band of the threshold', amax)
    return amax >= THRESH


class Cnl:
    """K3 on one weight set: every call packs afresh (the pack zeroes the status word)."""
    def __init__(self, st):
        from humannerf_amd import ops
        self.ops, self.lists = ops, cnl_lists(st)

    def pack(self):
        return self.ops.canonical_pack(*self.lists, 'f16x3')

    def run(self, xyz, mode='f16x3', idx=None, count=None):
        packed = self.pack()
        if idx is None:
            out = self.ops.canonical(xyz, packed, mode)
        else:
            out = self.ops.canonical_sparse(xyz, packed, idx, count, mode)
        return out, int(self.ops.status_word(packed, 'canonical', 'f16x3').item())


class Nr:
    """K2 on one weight set and condition code."""
    def __init__(self, st, cond):
        from humannerf_amd import ops
        self.ops, self.lists = ops, nr_lists(st)
        self.cond = torch.from_numpy(cond).to(dev())

    def pack(self):
        return self.ops.nonrigid_pack(*self.lists, self.cond, 'f16x3')

    def run(self, x, hw, mode='f16x3', idx=None, count=None):
        packed = self.pack()
        if idx is None:
            out = self.ops.nonrigid(x, hw, packed, mode, want_offsets=True)[1]
        else:
            out = self.ops.nonrigid_sparse(x, hw, packed, idx, count, mode)
        return out, int(self.ops.status_word(packed, 'nonrigid', 'f16x3').item())


def _hann():
    from oracle import oracle
    return oracle.hann_weights(1e7, 6, 10000, 50000)


def _inputs(P, seed, hot=None):
    """P sample positions in [-1.3, 0.9]^3 (``hot``: these sample numbers get x = 1.2) and a condition code."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1.3, 0.9, (P, 3)).astype(np.float32)
    if hot is not None:
        x[hot, 0] = 1.2
    return x, rs.uniform(-0.5, 0.5, (69,)).astype(np.float32)


def _gate(mlp):
    """``plant``'s gate: GATE at x = 1.2, 0 for x <= 0.9 (canonical: PE column 0 is x itself; non-rigid: sin(x),
    column 69 of [cond, pe], hann weights 1)."""
    if mlp == 'cnl':
        col, lo, hi = 0, 1.0, 1.2
    else:
        col, lo, hi = 69, np.sin(1.05), np.sin(1.2)
    s = GATE / (hi - lo)
    return col, s, -s * lo


# ------------------------------------------------------------------ 2. sensitivity and specificity, kernel level
FEATS = {'cnl': [0, 3, 4, 31, 32, 224, 255], 'nr': [0, 4, 31, 96, 127]}
VALUES = [100.0, 140.0, 5.0e4, 1.0e5]


@pytest.mark.parametrize('mlp,l', [('cnl', l) for l in range(8)] + [('nr', l) for l in range(6)])
def test_guard_sees_every_layer_feature_and_value(mlp, l):
    """Every hidden layer, features at both ends of a tile, both lane halves and in the last tile of the layer (the
    deferred epilogue): 100 raises nothing, 140, 5e4 and 1e5 (clamped) raise the word; '+noguard' leaves the word at 0
    and gives the same bits, hit or not.  P = 333 leaves the last workgroup partial."""
    P = 333
    x, cond = _inputs(P, 10 + l)
    xt, hw = torch.from_numpy(x).to(dev()), _hann().to(dev())
    base = _mlp_states(np.random.RandomState(100 + l))
    for j in FEATS[mlp]:
        for v in VALUES:
            st = plant(base, mlp, l, j, v)
            if mlp == 'cnl':
                k, amax = Cnl(st), oracle_cnl(st, x)[1]
                run = lambda mode: k.run(xt, mode)
            else:
                k, amax = Nr(st, cond), oracle_nr(st, x, cond, _hann())[1]
                run = lambda mode: k.run(xt, hw, mode)
            out, word = run('f16x3')
            assert word == (1 if expect_hit(amax) else 0), (mlp, l, j, v, amax, word)
            assert torch.isfinite(out).all()
            out_ng, word_ng = run('f16x3+noguard')
            assert word_ng == 0, (mlp, l, j, v)
            assert torch.equal(out, out_ng), (mlp, l, j, v)


@pytest.mark.parametrize('mlp,l', [('cnl', 1), ('cnl', CNL_SKIP), ('cnl', 7), ('nr', 1), ('nr', NR_SKIP), ('nr', 5)])
@pytest.mark.parametrize('value', [100.0, 1.0e5])
def test_guard_one_hot_sample_in_the_last_workgroup(mlp, l, value):
    """Only the last sample of a ragged P reaches ``value`` (gated by its x): the dense and the sparse forms
    raise exactly when that sample is evaluated and the fp64 activations say so; '+noguard' raises nothing and keeps
    the bits."""
    from humannerf_amd import ops
    P = 4133
    x, cond = _inputs(P, 5, hot=[P - 1])
    st = plant(_mlp_states(np.random.RandomState(7)), mlp, l, 17, value, gate=_gate(mlp))
    xt, hw = torch.from_numpy(x).to(dev()), _hann().to(dev())
    if mlp == 'cnl':
        k, (_, amax) = Cnl(st), oracle_cnl(st, x)
        _, amax_cold = oracle_cnl(st, x[:-1])
        run = lambda mode, **kw: k.run(xt, mode, **kw)
    else:
        k, (_, amax) = Nr(st, cond), oracle_nr(st, x, cond, _hann())
        _, amax_cold = oracle_nr(st, x[:-1], cond, _hann())
        run = lambda mode, **kw: k.run(xt, hw, mode, **kw)
    hit = expect_hit(amax)
    assert hit == (value > THRESH) and not expect_hit(amax_cold)
    dense, word = run('f16x3')
    assert word == int(hit)
    dense_ng, word_ng = run('f16x3+noguard')
    assert word_ng == 0 and torch.equal(dense, dense_ng)
    every = torch.arange(P, dtype=torch.int32, device=dev())
    for idx, n, want in ((every, P, hit), (every[:-1].contiguous(), P - 1, False),
                         (every.flip(0).contiguous(), P, hit), (every[-1:].contiguous(), 1, hit)):
        count = torch.tensor([n], dtype=torch.int32, device=dev())
        _, word = run('f16x3', idx=idx, count=count)
        assert word == int(want), (n, want)
        _, word = run('f16x3+noguard', idx=idx, count=count)
        assert word == 0


# ------------------------------------------------------------------ 3. accuracy envelope below the threshold
def _check_cnl(st, x, mode, tag):
    """K3 against fp64, with the bounds of test_gpu_parity.test_canonical_mlp_kernel.  Returns the relative error."""
    from humannerf_amd import ops
    ws, bs = cnl_lists(st)
    packed = ops.canonical_pack(ws, bs, mode)
    raw = ops.canonical(torch.from_numpy(x).to(dev()), packed, mode).cpu().numpy()
    ref64, amax = oracle_cnl(st, x)
    ref32, _ = oracle_cnl(st, x, torch.float32)
    scale = max(1.0, np.abs(ref64).max())
    e_hip, e_cpu = np.abs(raw - ref64).max() / scale, np.abs(ref32 - ref64).max() / scale
    print('canonical', mode, tag, 'max act %.3g rel err hip %.2e cpu-fp32 %.2e' % (amax, e_hip, e_cpu))
    return amax, e_hip, e_cpu


def _check_nr(st, x, cond, mode, tag):
    """K2 against fp64, with the bounds of test_gpu_parity.test_nonrigid_mlp_kernel."""
    from humannerf_amd import ops
    hw = _hann()
    ws, bs = nr_lists(st)
    packed = ops.nonrigid_pack(ws, bs, torch.from_numpy(cond).to(dev()), mode)
    _, ofs = ops.nonrigid(torch.from_numpy(x).to(dev()), hw.to(dev()), packed, mode, want_offsets=True)
    ref64, amax = oracle_nr(st, x, cond, hw)
    ref32, _ = oracle_nr(st, x, cond, hw, torch.float32)
    top = float(np.abs(ref64).max())
    e_hip = float(np.abs(ofs.cpu().numpy() - ref64).max()) / top
    e_cpu = float(np.abs(ref32.astype(np.float64) - ref64).max()) / top
    print('nonrigid', mode, tag, 'max act %.3g max|offset| %.2e rel err hip %.2e cpu-fp32 %.2e'
          % (amax, top, e_hip, e_cpu))
    return amax, e_hip, e_cpu


def _cnl_regime(st, regime, rs):
    """Weight regimes of the canonical MLP, mirroring test_gpu_parity._apply_regime for K2:
      head_tiny    output layer x 1e-5 (pack_layer16's head_scale lifts it by 2^14)
      head_large   output layer x 32 (lowered by a negative power of two)
      tiny_hidden  a hidden layer (pts_linears.6) with weights and biases ~1e-6 (layer_exponent)
      fresh_init   output layer U(+-1e-5), zero bias: every hi of the head is an f16 subnormal before the lift."""
    h = CNL_HEAD
    if regime == 'head_tiny':
        st[h + '.weight'] *= np.float32(1e-5)
        st[h + '.bias'] *= np.float32(1e-5)
    elif regime == 'head_large':
        st[h + '.weight'] *= np.float32(32.0)
    elif regime == 'tiny_hidden':
        st[CNL + '6.weight'] *= np.float32(1e-5)
        st[CNL + '6.bias'] *= np.float32(1e-5)
    elif regime == 'fresh_init':
        st[h + '.weight'] = rs.uniform(-1e-5, 1e-5, st[h + '.weight'].shape).astype(np.float32)
        st[h + '.bias'] = np.zeros_like(st[h + '.bias'])
    else:
        raise ValueError(regime)
    return st


@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
@pytest.mark.parametrize('regime', ['head_tiny', 'head_large', 'tiny_hidden', 'fresh_init'])
@pytest.mark.parametrize('P', [97, 2048])
def test_canonical_mlp_weight_regimes(P, regime, mode):
    """K3 in the weight regimes K2 is tested in: as accurate as CPU fp32, relative to the output magnitude."""
    rs = np.random.RandomState(P + 3)
    st = _cnl_regime(_mlp_states(rs), regime, rs)
    x = rs.uniform(-1.3, 1.3, (P, 3)).astype(np.float32)
    _, e_hip, e_cpu = _check_cnl(st, x, mode, regime)
    scale = max(1e-30, float(np.abs(oracle_cnl(st, x)[0]).max()))
    if scale < 1.0:                       # (the bound above is relative to max(1, |raw|): also relative to |raw| itself)
        e_hip, e_cpu = e_hip / scale, e_cpu / scale
    assert e_hip <= 2e-5, (e_hip, e_cpu)
    assert e_hip <= 4 * e_cpu + 1e-6, (e_hip, e_cpu)


CARRY = 0.5                 # what a carried activation contributes to each row of the layer that reads it
CARRIED = [1e2, 120.0, 1e3, 1e4, 5e4]
SITES = {'cnl': [(3, 100), (CNL_SKIP - 1, 7), (7, 255)], 'nr': [(1, 50), (NR_SKIP - 1, 3), (5, 127)]}


@pytest.mark.parametrize('mode', ['f32', 'f16x3'])
@pytest.mark.parametrize('value', CARRIED)
@pytest.mark.parametrize('mlp', ['cnl', 'nr'])
def test_carried_activation_accuracy(mlp, value, mode):
    """An activation of ``value`` that takes part in the output (outgoing weights CARRY / value): 'f32' matches fp64
    to the bounds of the kernel tests in test_gpu_parity at every size; 'f16x3' does below the guard's threshold and
    raises the status word above it (the contract: no hit -> fp32 accuracy).  Before the threshold came down to 128,
    1e3 went unreported with 2.3e-5 of error in both MLPs, 5e4 with 6.8e-4: a weight's low part is stored un-lifted,
    so |w| < 0.25 keeps an absolute error of up to 2^-25, which the activation multiplies."""
    rs = np.random.RandomState(int(value) % 1000 + 11)
    base = _mlp_states(rs)
    P = 1000
    x = rs.uniform(-1.3, 1.3, (P, 3)).astype(np.float32)
    cond = rs.uniform(-0.5, 0.5, (69,)).astype(np.float32)
    for l, j in SITES[mlp]:
        st = plant(base, mlp, l, j, value, carry=CARRY / value)
        tag = 'carried %g layer %d feature %d' % (value, l, j)
        if mlp == 'cnl':
            amax, e_hip, e_cpu = _check_cnl(st, x, mode, tag)
            bound = (2e-5, 4.0, 1e-6)
        else:
            amax, e_hip, e_cpu = _check_nr(st, x, cond, mode, tag)
            bound = (1e-5, 8.0, 2e-7)
        hit = expect_hit(amax)
        if mode == 'f16x3':
            if mlp == 'cnl':
                _, word = Cnl(st).run(torch.from_numpy(x).to(dev()))
            else:
                _, word = Nr(st, cond).run(torch.from_numpy(x).to(dev()), _hann().to(dev()))
            assert word == int(hit), (tag, amax, word)
            if hit:
                continue
        assert e_hip <= bound[0], (tag, e_hip, e_cpu)
        assert e_hip <= bound[1] * e_cpu + bound[2], (tag, e_hip, e_cpu)


# ------------------------------------------------------------------ 4. routing through the entry points
def _scene(R, S, hot_rays, hot_axis=0, hot_lo=0.6, fg_hot=None, seed=3):
    """Rays along +z through [-1, 1] in z under the identity motion (canonical x == world x, no non-rigid MLP):
    the rays numbered ``hot_rays`` have coordinate ``hot_axis`` in [hot_lo, hot_lo + 0.1], the others stay below
    0.3.  ``fg_hot``: bone weight of every bone at x > 0.5 (else 0.04 everywhere)."""
    rs = np.random.RandomState(seed)
    d = dev()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(d)
    B, G = 24, 32
    o = np.zeros((R, 3))
    o[:, :2] = rs.uniform(-0.9, 0.3, (R, 2))
    o[:, 2] = -3.0
    o[hot_rays, hot_axis] = rs.uniform(hot_lo, hot_lo + 0.1, len(hot_rays))
    dirs = np.tile([0.0, 0.0, 1.0], (R, 1))
    vol = np.full((B + 1, G, G, G), 0.04)
    if fg_hot is not None:
        vol[:B, :, :, 22:] = fg_hot                # vol[c][z][y][x]: voxel 22 of 32 over [-1.2, 1.2] sits at x = 0.5
    args = dict(rays_o=T(o), rays_d=T(dirs), near=T(np.full(R, 2.0)), far=T(np.full(R, 4.0)), t_rand=None,
                motion_Rs=T(np.tile(np.eye(3), (B, 1, 1))), motion_Ts=T(np.zeros((B, 3))), vol=T(vol),
                bbox_min=T(np.full(3, -1.2)), bbox_scale=T(np.full(3, 2.0 / 2.4)), hann_w=None, nr_packed=None)
    return args, T(np.array([255., 128., 0.])), S


def _hot_canonical(axis=0, slope=100.0, offset=-50.0, head_sigma=0.0, st=None, seed=21):
    """Canonical weights whose layer-1 feature 9 is 1e4 relu(slope * p + offset) of coordinate ``axis`` (>= 1e5
    where the gate reaches GATE: p >= 0.6 by default; 0 for p <= 0.5); its outgoing column is zero (only the guard can
    see it)."""
    st = plant(_mlp_states(np.random.RandomState(seed)) if st is None else st, 'cnl', 1, 9, 1e5,
               gate=(axis, slope, offset))
    st[CNL_HEAD + '.bias'][3] += np.float32(head_sigma)
    return st


def test_render_frame_guard_routing():
    """hnrf_render_frame_fwd on 4 chunks, the hot rays all in chunk j: a plain mode raises the word, '+guard1:k'
    raises it iff k % 4 == j, '+noguard' never; rgb / alpha / depth are the same bits in every mode."""
    from humannerf_amd import ops
    R, chunk, j = 4096, 1024, 2
    args, bg, S = _scene(R, 64, list(range(j * chunk + 100, j * chunk + 110)))
    ws, bs = cnl_lists(_hot_canonical())

    def frame(mode):
        packed = ops.canonical_pack(ws, bs, 'f16x3')
        out, _ = ops.render_frame(*args.values(), packed, bg, S, chunk, mode, diagnostics=False)
        return out, int(ops.status_word(packed, 'canonical', 'f16x3').item())

    ref, word = frame('f16x3')
    assert word == 1
    for mode, want in [('f16x3+noguard', 0)] + [('f16x3+guard1:%d' % k, int(k % 4 == j)) for k in range(9)]:
        out, word = frame(mode)
        assert word == want, mode
        for key in ('rgb', 'alpha', 'depth'):
            assert torch.equal(out[key], ref[key]), (mode, key)
    # the same frame without the hot rays raises nothing in any mode
    cold, bg, S = _scene(R, 64, [])
    packed = ops.canonical_pack(ws, bs, 'f16x3')
    ops.render_frame(*cold.values(), packed, bg, S, chunk, 'f16x3', diagnostics=False)
    assert int(ops.status_word(packed, 'canonical', 'f16x3').item()) == 0


@pytest.mark.parametrize('entry', ['frame', 'rays'])
def test_culled_hot_samples_raise_nothing(entry):
    """cull_eps > 0: the hot samples sit where the bone weights sum to 2.4e-4 and are culled -- never evaluated, no
    hit; with cull_eps = 0 the same samples raise the word."""
    from humannerf_amd import ops
    R = 2048
    args, bg, S = _scene(R, 64, list(range(500, 520)), fg_hot=1e-5)
    ws, bs = cnl_lists(_hot_canonical())
    for eps, want in ((1e-3, 0), (0.0, 1)):
        packed = ops.canonical_pack(ws, bs, 'f16x3')
        if entry == 'frame':
            ops.render_frame(*args.values(), packed, bg, S, 1024, 'f16x3', diagnostics=False, cull_eps=eps)
        else:
            ops.render_rays(*args.values(), packed, bg, S, 'f16x3', cull_eps=eps,
                            workspace=torch.empty(ops.render_workspace_bytes(R, S) // 4 + 64, device=dev()))
        assert int(ops.status_word(packed, 'canonical', 'f16x3').item()) == want, eps


def test_early_termination_skips_hot_samples_behind_saturated_rays():
    """A dense medium saturates every ray in its first slab of 32 samples: a hot sample at the far end (z > 0.6) is
    never evaluated by hnrf_render_rays_term_fwd and raises nothing (the dense path does raise it); a hot sample at
    the near end (z < -0.8) raises the word."""
    from humannerf_amd import ops
    R, S = 1024, 128
    args, bg, _ = _scene(R, S, [])
    for where, slope, offset, want in (('far', 100.0, -60.0, 0), ('near', -100.0, -80.0, 1)):
        # the gate on z: hot for z >= 0.7 (0 below 0.6), or for z <= -0.9 (0 above -0.8); sigma >= 37 everywhere: a
        # ray saturates within its first 32 samples (z < -0.5)
        ws, bs = cnl_lists(_hot_canonical(axis=2, slope=slope, offset=offset, head_sigma=40.0))
        packed = ops.canonical_pack(ws, bs, 'f16x3')
        out = ops.render_rays_term(*args.values(), packed, bg, S, 'f16x3', term_eps=1e-4, want_count=True)
        assert int(ops.status_word(packed, 'canonical', 'f16x3').item()) == want, where
        assert int(out['evaluated'].item()) < R * S // 2
        assert float(out['alpha'].min()) > 0.99
        packed = ops.canonical_pack(ws, bs, 'f16x3')
        ops.render_rays(*args.values(), packed, bg, S, 'f16x3',
                        workspace=torch.empty(ops.render_workspace_bytes(R, S) // 4 + 64, device=dev()))
        assert int(ops.status_word(packed, 'canonical', 'f16x3').item()) == 1     # reachable without termination


@pytest.fixture
def hot_net(seeded_params):
    """The seeded network with _hot_canonical's feature: canonical x >= 0.6 is out of range."""
    from humannerf_amd.network import Network
    st = _hot_canonical(st=dict(seeded_params))
    net = Network()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    return net.to(dev()).eval()


def test_density_grid_guard(hot_net, golden_frame):
    """hnrf_density_grid raises the word for a hot lattice point inside the bbox; Network.canonical_density_grid
    raises ActivationRangeError under 'raise' and returns the grid of an 'f32' network under 'f32'."""
    from humannerf_amd import ops
    from humannerf_amd.config import cfg
    from humannerf_amd.network import ActivationRangeError
    fr = golden_frame
    bmin, bmax = fr['cnl_bbox_min_xyz'], fr['cnl_bbox_max_xyz']
    assert bmin[0] < 0.4 and bmax[0] > 0.7
    net = hot_net
    mr, mt, vol = net.frame_motion(fr)
    f = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dev()).contiguous()
    packed = net._canonical_packed()
    ops.density_grid(packed, vol, f(bmin), f(bmax), f(fr['cnl_bbox_scale_xyz']), 32, 'f16x3')
    assert int(ops.status_word(packed, 'canonical', 'f16x3').item()) == 1
    try:
        cfg.amd.mlp_mode = 'f16x3'
        net.f16_guard.reset()
        with pytest.raises(ActivationRangeError, match='canonical'):
            net.canonical_density_grid(bmin, bmax, fr['motion_weights_priors'], resolution=32)
        cfg.amd.on_f16_range = 'f32'
        net.f16_guard.reset()
        with pytest.warns(UserWarning, match="switching this network to 'f32'"):
            grid = net.canonical_density_grid(bmin, bmax, fr['motion_weights_priors'], resolution=32)
        assert net._mlp_mode() == 'f32'
        cfg.amd.mlp_mode, cfg.amd.on_f16_range = 'f32', 'raise'
        net.f16_guard.reset()
        want = net.canonical_density_grid(bmin, bmax, fr['motion_weights_priors'], resolution=32)
        assert torch.equal(grid, want)
    finally:
        cfg.amd.mlp_mode, cfg.amd.on_f16_range = 'f16x3', 'raise'
        net.f16_guard.reset()


# ------------------------------------------------------------------ 5. the frame loop under each policy
@pytest.mark.parametrize('policy', ['raise', 'f32', 'ignore'])
def test_render_frames_under_each_policy(policy, hot_net, monkeypatch):
    """render.render_frames on 6 frames of a checkpoint whose activations leave the f16 range.  'raise': ends with
    ActivationRangeError.  'f32': every frame is delivered once and equals an 'f32' render.  'ignore': every frame is
    delivered once and rendered once."""
    from humannerf_amd import render, scene
    from humannerf_amd.config import cfg
    from humannerf_amd.network import ActivationRangeError
    frames = [scene.synthetic_frame(H=40, W=40, focal_at_512=1250.0, pose_seed=s) for s in range(6)]
    net = hot_net
    calls, delivered = [], []
    fwd = net.forward

    def counting(*a, **k):
        calls.append(1)
        return fwd(*a, **k)

    def on_image(i, rgb8, a8):
        delivered.append((i, rgb8.copy()))

    cfg.amd.diagnostics = False
    try:
        cfg.amd.mlp_mode = 'f32'
        want = render.render_frames(net, frames)
        cfg.amd.mlp_mode, cfg.amd.on_f16_range = 'f16x3', policy
        net.f16_guard.reset()
        net._drop(lambda e: e.packed is not None)
        monkeypatch.setattr(net, 'forward', counting)
        if policy == 'raise':
            with pytest.raises(ActivationRangeError):
                render.render_frames(net, frames, on_image=on_image)
            return
        if policy == 'f32':
            with pytest.warns(UserWarning, match="switching this network to 'f32'"):
                got = render.render_frames(net, frames, on_image=on_image)
        else:
            got = render.render_frames(net, frames, on_image=on_image)
            assert net.f16_range_hits >= 1
            assert len(calls) == len(frames)
        assert sorted(i for i, _ in delivered) == list(range(len(frames)))
        for i, img in delivered:
            assert np.array_equal(img, got[i])
        if policy == 'f32':
            for i in range(len(frames)):
                assert np.array_equal(got[i], want[i]), i
    finally:
        cfg.amd.diagnostics, cfg.amd.mlp_mode, cfg.amd.on_f16_range = True, 'f16x3', 'raise'
        net.f16_guard.reset()
        net._drop(lambda e: e.packed is not None)
