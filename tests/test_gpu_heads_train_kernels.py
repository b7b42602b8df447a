"""The all-heads training kernels (include/hnrf_heads_train.h) against the single-head kernels, bit for bit where the
header says so, and against fp64 at the bounds of tests/test_gpu_train_kernels.py (``tk``), whose helpers and
references this module drives with a (4H, 256) head layer.  Shapes: H in 2, 3, 5, 8 (one (q, half) pair, an empty half,
past the split-f16 k-step boundary 4 H > 16, the full tile) by sample counts around the 128-sample workgroup."""
import numpy as np
import pytest
import torch

from tests import test_gpu_train_kernels as tk
from tests.heads_train_cases import HEAD_COUNTS, head_problem, make_heads_problem, wide_gradient
from tests.test_gpu_grad import _rows
from tests.test_train_kernel_refs import SPECS, ref_mlp_grads, ref_weight_grads_from_operands

pytestmark = pytest.mark.gpu

MODES = tk.MODES
SPEC = SPECS['canonical']
T, _buf, _pad128 = tk.T, tk._buf, tk._pad128


def gpu_heads_forward(pr, mode, fill=None):
    """hnrf_canonical_heads_fwd_train through the C ABI -> dict(out (H, P, 4), pe, acts, bits, ws, x)."""
    from humannerf_amd import _lib, ops
    lib = _lib.load_heads_train()
    H, P, half = pr['H'], pr['P'], mode == 'f16x3h'
    ws, bs = [T(w) for w in pr['ws']], [T(b) for b in pr['bs']]
    x = T(pr['x'])
    packed = ops.canonical_heads_pack(ws, bs, H, 'f16x3' if half else mode)
    out = _buf((H, P, 4), torch.float32, fill)
    pe = _buf((P, 64), torch.float16, fill) if half else _buf((P, 63), torch.float32, fill)
    acts = _buf((8, _pad128(P), 256), torch.float16, fill) if half else _buf((8, P, 256), torch.float32, fill)
    bits = _buf((8, P, 8), torch.int32, fill)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.hnrf_canonical_heads_fwd_train(x.data_ptr(), packed.data_ptr(), ops.TRAIN_MODES[mode], P, H, out.data_ptr(),
                                                  pe.data_ptr(), acts.data_ptr(), bits.data_ptr(), st),
               'hnrf_canonical_heads_fwd_train')
    torch.cuda.synchronize()
    return dict(out=out, offsets=None, pe=pe, acts=acts, bits=bits, ws=ws, x=x)


def gpu_heads_backward(pr, mode, fwd, g=None, fill=None, amax_in=None):
    """hnrf_canonical_heads_bwd through the C ABI -> dict(dZ, d_x, amax, g (H, P, 4)), as tk.gpu_backward."""
    from humannerf_amd import _lib, ops
    lib = _lib.load_heads_train()
    H, P, half = pr['H'], pr['P'], mode == 'f16x3h'
    g = T(pr['g'] if g is None else g)
    m = ops.MLP_MODES['f16x3' if half else mode]
    st = torch.cuda.current_stream().cuda_stream
    nbytes = lib.hnrf_canonical_heads_bwd_packed_bytes(m, H)
    assert nbytes > 0
    packed = torch.empty((nbytes + 3) // 4, device=tk.dev())
    _lib.check(lib.hnrf_canonical_heads_bwd_pack(ops._ptr_array(fwd['ws']), H, m, packed.data_ptr(), st), 'heads_bwd_pack')
    if mode == 'f32':
        am = None
    elif amax_in is None:
        am = g.abs().amax().reshape(1)
    else:
        am = torch.tensor([amax_in], dtype=torch.float32, device=tk.dev())
    dZ = _buf((8, _pad128(P), 256), torch.float16, fill) if half else _buf((8, P, 256), torch.float32, fill)
    d_x = _buf((P, 3), torch.float32, fill)
    amax = _buf((8,) if half else (8, 64), torch.float32, fill)
    _lib.check(lib.hnrf_canonical_heads_bwd(fwd['x'].data_ptr(), g.data_ptr(), fwd['bits'].data_ptr(), packed.data_ptr(),
                                            ops.TRAIN_MODES[mode], ops._ptr(am), P, H, dZ.data_ptr(), d_x.data_ptr(),
                                            amax.data_ptr(), st), 'hnrf_canonical_heads_bwd')
    torch.cuda.synchronize()
    return dict(dZ=dZ, d_x=d_x, amax=amax, g=g)


def _rel(a, b):
    a = a.double().cpu()
    top = float(b.abs().max())
    if top == 0.0:
        return 0.0 if float(a.abs().max()) == 0.0 else float('inf')
    return float((a - b).abs().max() / top)


def check_heads_backward(pr, mode, g=None, amax_in=None, label='', fwd=None):
    """tk.check_backward for the all-heads chain: forward-train -> chain -> weight gradients (the training step's glue,
    the head layer once per plane) against fp64 autograd through the (4H, 256) head with the kernel's sign pattern.  The
    head layer's rows are compared per head, each against its own largest element."""
    H, P, half = pr['H'], pr['P'], mode == 'f16x3h'
    g = pr['g'] if g is None else g
    fwd = gpu_heads_forward(pr, mode) if fwd is None else fwd
    bwd = gpu_heads_backward(pr, mode, fwd, g=g, amax_in=amax_in)
    gW, gb = tk.gpu_weight_grads(pr, mode, fwd, bwd)
    assert tuple(gW[8].shape) == (4 * H, 256) and tuple(gb[8].shape) == (4 * H,)
    ref = ref_mlp_grads(pr, tk.masks_of(fwd, P, half), wide_gradient(g))
    errs = tk.rel_errors(pr, ref, bwd['d_x'], gW[:8], gb[:8])
    for h in range(H):
        r = slice(4 * h, 4 * h + 4)
        errs['W8h%d' % h], errs['b8h%d' % h] = _rel(gW[8][r], ref['dW'][8][r]), _rel(gb[8][r], ref['db'][8][r])
    dZ = tk.rows(bwd['dZ'], P, half)
    for l in range(8):
        got = dZ[l] / float(bwd['amax'][l]) if half else dZ[l]
        errs['dZ%d' % l] = _rel(got, ref['dZ'][l])
    if half:
        assert bwd['dZ'].dtype == torch.float16 and bwd['amax'].shape == (8,)
        sc = bwd['amax'].cpu()
        assert bool(torch.isfinite(sc).all()) and float(sc.min()) > 0
        assert all(float(torch.log2(a)) == round(float(torch.log2(a))) for a in sc)             # powers of two
        full = [_rows(bwd['dZ'][l], _pad128(P), True) for l in range(8)]
        assert all(float(f[P:].abs().max()) == 0.0 for f in full if f.shape[0] > P)            # padded rows: zeros
        scale = bwd['amax'].double().cpu()
        oW, ob = ref_weight_grads_from_operands(SPEC, [z / scale[l] for l, z in enumerate(dZ)], tk.rows(fwd['acts'], P, True),
                                                fwd['pe'].double().cpu()[:, :63], torch.from_numpy(wide_gradient(g)).double())
        for l in range(8):
            errs['op_W%d' % l], errs['op_b%d' % l] = _rel(gW[l], oW[l]), _rel(gb[l], ob[l])
        for h in range(H):
            r = slice(4 * h, 4 * h + 4)
            errs['op_W8h%d' % h], errs['op_b8h%d' % h] = _rel(gW[8][r], oW[8][r]), _rel(gb[8][r], ob[8][r])
    else:
        assert torch.equal(bwd['amax'].amax(1), bwd['dZ'].abs().amax(dim=(1, 2)))
    print('heads backward H=%d' % H, mode, P, label, 'worst %.2e (%s)' % max((v, k) for k, v in errs.items()))
    return errs, fwd, bwd


# ------------------------------------------------------------------------------------------------------- forward
def assert_forward_equals_single_head(pr, mode, fwd):
    """The bit-identity contract: pe, acts, the sign masks and every plane of raw equal hnrf_canonical_fwd_train on the
    single-head image of that head's four rows."""
    P, half = pr['P'], mode == 'f16x3h'
    for h in range(pr['H']):
        one = tk.gpu_forward(head_problem(pr, h), mode)
        assert torch.equal(fwd['out'][h], one['out']), ('raw', h)
        assert torch.equal(fwd['pe'], one['pe']) and torch.equal(fwd['bits'], one['bits']), h
        for l in range(8):
            assert torch.equal(_rows(fwd['acts'][l], P, half), _rows(one['acts'][l], P, half)), (h, l)
        if half:                                                          # padding rows of the blocked layers too
            assert torch.equal(fwd['acts'], one['acts']), h


@pytest.mark.parametrize('P', [1, 127, 128, 129, 777])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('H', HEAD_COUNTS)
def test_all_heads_forward_equals_single_head_forward_and_matches_fp64(H, mode, P):
    """canonical_f32_kernel<true, true> / canonical_f16x3_kernel<SV_ACT | SV_ACT_H, false, true>: everything the
    single-head instance saves, bit for bit, every plane of raw bit for bit, and every plane with the saved state against
    fp64 at tk's bounds (raw 2e-5 max(1, max|raw|), activations 2e-5 max(1, max|h|), the f16-stored forms as tk states)."""
    pr = make_heads_problem(H, P, 100 * H + P)
    fwd = gpu_heads_forward(pr, mode)
    assert_forward_equals_single_head(pr, mode, fwd)
    for h in range(H):
        tk.check_forward(head_problem(pr, h), mode, dict(fwd, out=fwd['out'][h]), label='head %d of %d' % (h, H))


@pytest.mark.parametrize('mode', MODES)
def test_head_of_tiny_weights_next_to_normal_ones_keeps_its_own_descale(mode):
    """One head at +-1e-5 between normal ones ("The descale trap"): the multi-head image lifts
    every head by a power of two of its own, so the tiny head loses nothing to its neighbours and still equals the
    single-head kernel bit for bit."""
    pr = make_heads_problem(3, 129, 4242, tiny_head=1)
    fwd = gpu_heads_forward(pr, mode)
    assert 0.0 < float(fwd['out'][1].abs().max()) < 1e-3 < float(fwd['out'][0].abs().max())
    assert_forward_equals_single_head(pr, mode, fwd)
    for h in range(3):
        tk.check_forward(head_problem(pr, h), mode, dict(fwd, out=fwd['out'][h]), label='tiny head 1, head %d' % h)


# ------------------------------------------------------------------------------------- chain and weight gradients
@pytest.mark.parametrize('P', [1, 127, 129, 777])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('H', HEAD_COUNTS)
def test_all_heads_chain_and_weight_gradients_match_fp64(H, mode, P):
    """canonical_bwd_kernel<true> / canonical_bwd16_kernel<false | true, true> and the per-plane head gradients: d_xyz 2e-5,
    dZ 2e-5 (+ 2^-11 f16-stored), dW / db 2e-5 (fp32 operands) or 1e-3 (f16 operands; 2e-6 against the fp64 product of
    the saved operands), the head layer's rows per head."""
    pr = make_heads_problem(H, P, 3000 + 100 * H + P)
    errs, _, _ = check_heads_backward(pr, mode)
    tk.assert_backward_bounds(errs, mode, (H, P))


@pytest.mark.parametrize('P', [1, 127, 129, 777])
@pytest.mark.parametrize('H', HEAD_COUNTS)
def test_one_hot_gradient_equals_the_single_head_chain_in_f32(H, P):
    """Mode 'f32', d_raw zero outside plane h: the other heads contribute exact zero products, so d_xyz and dZ compare
    equal (==: a zero's sign may differ) to hnrf_canonical_bwd on head h's rows -- for every h, i.e. every (q, half)
    position of the head stage."""
    pr = make_heads_problem(H, P, 5000 + 100 * H + P)
    fwd = gpu_heads_forward(pr, 'f32')
    for h in range(H):
        g = np.zeros_like(pr['g'])
        g[h] = pr['g'][h]
        bwd = gpu_heads_backward(pr, 'f32', fwd, g=g)
        rows_h = fwd['ws'][-1][4 * h:4 * h + 4].contiguous()
        one = tk.gpu_backward(head_problem(pr, h), 'f32', dict(fwd, ws=fwd['ws'][:-1] + [rows_h]))
        assert bool((bwd['d_x'] == one['d_x']).all()), h
        assert bool((bwd['dZ'] == one['dZ']).all()), h
        assert bool((bwd['amax'] == one['amax']).all()), h


@pytest.mark.parametrize('mode', ['f16x3', 'f16x3h'])
@pytest.mark.parametrize('H', HEAD_COUNTS)
def test_one_hot_gradient_in_the_split_f16_modes_matches_fp64(H, mode):
    """The split-f16 head stage shares one exponent over all heads, which may differ from a single head's: the one-hot
    case is held to the fp64 bounds there (last head: the emptiest / the second k-step's position)."""
    pr = make_heads_problem(H, 129, 6000 + H)
    g = np.zeros_like(pr['g'])
    g[H - 1] = pr['g'][H - 1]
    errs, _, _ = check_heads_backward(pr, mode, g=g, label='one-hot %d' % (H - 1))
    tk.assert_backward_bounds(errs, mode, ('one-hot', H))


# ------------------------------------------------------------------------------------------ the amax contracts
AMAX_H, AMAX_P = 5, 777


@pytest.mark.parametrize('slack', [1.0, 1000.0])
@pytest.mark.parametrize('gscale', [2.0 ** -24, 1.0, 2.0 ** 10])
@pytest.mark.parametrize('mode', ['f16x3', 'f16x3h'])
def test_all_heads_backward_is_independent_of_the_gradient_scale(mode, gscale, slack):
    """tk.test_backward_is_independent_of_the_gradient_scale for the all-heads chain: d_raw_amax bounds all planes, may
    be 1000 x loose, and the same relative bounds hold at 2^-24, 1 and 2^10."""
    pr = make_heads_problem(AMAX_H, AMAX_P, 7000)
    g = pr['g'] * np.float32(gscale)
    amax_in = None if slack == 1.0 else float(np.abs(g).max()) * slack
    errs, _, _ = check_heads_backward(pr, mode, g=g, amax_in=amax_in, label='g x %g amax x %g' % (gscale, slack))
    tk.assert_backward_bounds(errs, mode, (gscale, slack))


@pytest.mark.parametrize('mode', ['f16x3', 'f16x3h'])
def test_all_heads_zero_gradient_gives_exact_zeros(mode):
    pr = make_heads_problem(AMAX_H, AMAX_P, 7100)
    fwd = gpu_heads_forward(pr, mode)
    bwd = gpu_heads_backward(pr, mode, fwd, g=pr['g'] * 0)
    gW, gb = tk.gpu_weight_grads(pr, mode, fwd, bwd)
    for t in [bwd['dZ'], bwd['d_x']] + list(gW) + list(gb):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0
    assert bool(torch.isfinite(bwd['amax']).all())
    if mode == 'f16x3h':
        assert float(bwd['amax'].min()) > 0
    else:
        assert float(bwd['amax'].abs().max()) == 0.0


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('mode', ['f16x3', 'f16x3h'])
def test_all_heads_non_finite_gradient_is_visible_in_every_output(mode, bad):
    """One inf / NaN in ONE plane: d_xyz and every hidden layer's dW / db fail isfinite().all(), and so do the rows of
    that plane's head (the other heads' rows are products of their own finite planes)."""
    pr = make_heads_problem(AMAX_H, AMAX_P, 7200)
    g = pr['g'].copy()
    g[3, 388, 1] = bad
    fwd = gpu_heads_forward(pr, mode)
    bwd = gpu_heads_backward(pr, mode, fwd, g=g)
    gW, gb = tk.gpu_weight_grads(pr, mode, fwd, bwd)
    assert not bool(torch.isfinite(bwd['d_x']).all())
    for l in range(8):
        assert not bool(torch.isfinite(gW[l]).all()), ('dW', l)
        assert not bool(torch.isfinite(gb[l]).all()), ('db', l)
    assert not bool(torch.isfinite(gW[8][12:16]).all()) and not bool(torch.isfinite(gb[8][12:16]).all())


# ------------------------------------------------------------------------------------------- buffer contents
def head_grads_direct(mode, P, H, fwd, bwd, fill):
    """The per-plane head calls of autograd._head_grads through the C ABI, output and workspace buffers of chosen contents."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    half = mode == 'f16x3h'
    st = torch.cuda.current_stream().cuda_stream
    gW, gb = _buf((4 * H, 256), torch.float32, fill), _buf((4 * H,), torch.float32, fill)
    X = fwd['acts'][7]
    for h in range(H):
        z, out, db = bwd['g'][h], gW[4 * h:4 * h + 4], gb[4 * h:4 * h + 4]
        if half:
            ws = _buf((lib.hnrf_mlp_dw_h_workspace_bytes(P, 4, 256),), torch.uint8, fill)
            _lib.check(lib.hnrf_mlp_dw_h(z.data_ptr(), z.stride(0), X.data_ptr(), X.stride(0), P, 4, 256, 2, 0, out.data_ptr(),
                                         out.stride(0), db.data_ptr(), ws.data_ptr(), ws.numel(), st), 'hnrf_mlp_dw_h')
        else:
            ws = _buf((lib.hnrf_mlp_dw_workspace_bytes(P, 4, 256),), torch.uint8, fill)
            _lib.check(lib.hnrf_mlp_dw(z.data_ptr(), z.stride(0), X.data_ptr(), X.stride(0), P, 4, 256, ops.MLP_MODES['f32'], 0, 0,
                                       out.data_ptr(), out.stride(0), db.data_ptr(), ws.data_ptr(), ws.numel(), st), 'hnrf_mlp_dw')
        torch.cuda.synchronize()
    return gW, gb


@pytest.mark.parametrize('P', [777, 1])
@pytest.mark.parametrize('mode', MODES)
def test_all_heads_results_do_not_depend_on_previous_buffer_contents(mode, P):
    """Forward-train -> chain -> the head's weight gradients once into zero-filled and once into NaN-poisoned output and
    workspace buffers: finite, bit-identical, and in 'f16x3h' the padded rows of the blocked dZ are exactly zero."""
    H = 5
    pr = make_heads_problem(H, P, 8000 + P)
    half = mode == 'f16x3h'
    runs = {}
    for fill in ('zero', 'poison'):
        fwd = gpu_heads_forward(pr, mode, fill)
        bwd = gpu_heads_backward(pr, mode, fwd, fill=fill)
        runs[fill] = (fwd, bwd) + head_grads_direct(mode, P, H, fwd, bwd, fill)
    (f0, b0, W0, B0), (f1, b1, W1, B1) = runs['zero'], runs['poison']
    for name in ('out', 'pe', 'bits'):
        assert torch.equal(f0[name], f1[name]), name
        assert f0[name].dtype == torch.int32 or bool(torch.isfinite(f1[name]).all()), name
    for l in range(8):
        for name, a, b in (('acts', f0['acts'][l], f1['acts'][l]), ('dZ', b0['dZ'][l], b1['dZ'][l])):
            ra, rb = _rows(a, P, half), _rows(b, P, half)
            assert bool(torch.isfinite(rb).all()) and torch.equal(ra, rb), (name, l)
        if half:
            pad = _rows(b1['dZ'][l], _pad128(P), True)[P:]
            assert pad.shape[0] == _pad128(P) - P and float(pad.abs().max()) == 0.0, l
            full = _rows(f1['acts'][l], _pad128(P), True)
            assert bool(torch.isfinite(full).all()) and torch.equal(full[P:], full[P - 1:P].expand(_pad128(P) - P, -1)), l
    assert torch.equal(b0['d_x'], b1['d_x']) and bool(torch.isfinite(b1['d_x']).all())
    assert torch.equal(b0['amax'], b1['amax']) and bool(torch.isfinite(b1['amax']).all())
    assert bool(torch.isfinite(W1).all()) and bool(torch.isfinite(B1).all())
    assert torch.equal(W0, W1) and torch.equal(B0, B1)
    gW, gb = tk.gpu_weight_grads(pr, mode, f0, b0)                         # and the direct calls are the glue's calls
    assert torch.equal(gW[8], W0) and torch.equal(gb[8], B0)
