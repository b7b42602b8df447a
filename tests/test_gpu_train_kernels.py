"""Every training-kernel instance against fp64, across sample counts, arithmetic modes, buffer contents and gradient
scales (DESIGN.md section 2 has the table of instances and the test that checks each one's values).

The kernels are driven through the C ABI with buffers this module allocates (so that their previous contents and
the amax argument can be chosen); the references are tests/test_train_kernel_refs.py: plain torch in fp64 on the
CPU.  The one thing a reference takes from the code under test is the ReLU sign pattern (the saved activations > 0)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_grad import _rows
from tests.test_train_kernel_refs import (SPECS, composite_problem, make_problem, ref_composite_grads, ref_mlp,
                                          ref_mlp_grads, ref_pe_grad, ref_weight_grads_from_operands)

pytestmark = pytest.mark.gpu

MODES = ['f32', 'f16x3', 'f16x3h']
KINDS = ['canonical', 'nonrigid']


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _buf(shape, dtype, fill):
    """An output / workspace buffer: fill None = as the allocator hands it out, 'zero', or 'poison' = f16 NaN 0x7E00,
    fp32 NaN, all bits set in integer buffers."""
    if fill is None:
        return torch.empty(shape, dtype=dtype, device=dev())
    if fill == 'zero':
        return torch.zeros(shape, dtype=dtype, device=dev())
    assert fill == 'poison'
    if dtype in (torch.int32, torch.uint8):
        return torch.full(shape, -1 if dtype == torch.int32 else 255, dtype=dtype, device=dev())
    t = torch.full(shape, float('nan'), dtype=dtype, device=dev())
    if dtype == torch.float16:
        assert int(t.view(torch.int16).flatten()[0]) == 0x7E00
    return t


def _pad128(P):
    return (P + 127) // 128 * 128


def gpu_forward(pr, mode, fill=None):
    """hnrf_*_fwd_train through the C ABI -> dict(out (raw | xyz), offsets, pe, acts, bits)."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    spec, P, half = SPECS[pr['kind']], pr['P'], mode == 'f16x3h'
    ws, bs = [T(w) for w in pr['ws']], [T(b) for b in pr['bs']]
    x = T(pr['x'])
    pmode = 'f16x3' if half else mode
    pe = _buf((P, 64), torch.float16, fill) if half else _buf((P, spec['npe']), torch.float32, fill)
    acts = (_buf((spec['L'], _pad128(P), spec['W']), torch.float16, fill) if half
            else _buf((spec['L'], P, spec['W']), torch.float32, fill))
    bits = _buf((spec['L'], P, spec['nb']), torch.int32, fill)
    st = torch.cuda.current_stream().cuda_stream
    if pr['kind'] == 'canonical':
        packed = ops.canonical_pack(ws, bs, pmode)
        out, offsets = _buf((P, 4), torch.float32, fill), None
        _lib.check(lib.hnrf_canonical_fwd_train(x.data_ptr(), packed.data_ptr(), ops.TRAIN_MODES[mode], P, out.data_ptr(),
                                                pe.data_ptr(), acts.data_ptr(), bits.data_ptr(), st), 'hnrf_canonical_fwd_train')
    else:
        packed = ops.nonrigid_pack(ws, bs, T(pr['cond']), pmode)
        out, offsets = _buf((P, 3), torch.float32, fill), _buf((P, 3), torch.float32, fill)
        _lib.check(lib.hnrf_nonrigid_fwd_train(x.data_ptr(), T(pr['hann']).data_ptr(), packed.data_ptr(), ops.TRAIN_MODES[mode], P,
                                               out.data_ptr(), offsets.data_ptr(), pe.data_ptr(), acts.data_ptr(),
                                               bits.data_ptr(), st), 'hnrf_nonrigid_fwd_train')
    torch.cuda.synchronize()
    return dict(out=out, offsets=offsets, pe=pe, acts=acts, bits=bits, ws=ws, x=x)


def gpu_backward(pr, mode, fwd, g=None, fill=None, amax_in=None):
    """hnrf_*_bwd through the C ABI -> dict(dZ, d_x, amax (fp32 modes: [L][64] maxima; 'f16x3h': [L] scales), g).
    amax_in: the d_raw_amax / d_xyz_amax argument (default: the true maximum of |g|)."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    spec, P, half = SPECS[pr['kind']], pr['P'], mode == 'f16x3h'
    g = T(pr['g'] if g is None else g)
    m = ops.MLP_MODES['f16x3' if half else mode]
    st = torch.cuda.current_stream().cuda_stream
    cn = pr['kind'] == 'canonical'
    nbytes = (lib.hnrf_canonical_bwd_packed_bytes if cn else lib.hnrf_nonrigid_bwd_packed_bytes)(m)
    packed = torch.empty((nbytes + 3) // 4, device=dev())
    _lib.check((lib.hnrf_canonical_bwd_pack if cn else lib.hnrf_nonrigid_bwd_pack)(ops._ptr_array(fwd['ws']), m, packed.data_ptr(), st),
               'bwd_pack')
    if mode == 'f32':
        am = None
    elif amax_in is None:
        am = g.abs().amax().reshape(1)
    else:
        am = torch.tensor([amax_in], dtype=torch.float32, device=dev())
    dZ = (_buf((spec['L'], _pad128(P), spec['W']), torch.float16, fill) if half
          else _buf((spec['L'], P, spec['W']), torch.float32, fill))
    d_x = _buf((P, 3), torch.float32, fill)
    amax = _buf((spec['L'],) if half else (spec['L'], 64), torch.float32, fill)
    if cn:
        _lib.check(lib.hnrf_canonical_bwd(fwd['x'].data_ptr(), g.data_ptr(), fwd['bits'].data_ptr(), packed.data_ptr(),
                                          ops.TRAIN_MODES[mode], ops._ptr(am), P, dZ.data_ptr(), d_x.data_ptr(), amax.data_ptr(), st),
                   'hnrf_canonical_bwd')
    else:
        _lib.check(lib.hnrf_nonrigid_bwd(fwd['x'].data_ptr(), T(pr['hann']).data_ptr(), g.data_ptr(), fwd['bits'].data_ptr(),
                                         packed.data_ptr(), ops.TRAIN_MODES[mode], ops._ptr(am), P, dZ.data_ptr(), d_x.data_ptr(),
                                         amax.data_ptr(), st), 'hnrf_nonrigid_bwd')
    torch.cuda.synchronize()
    return dict(dZ=dZ, d_x=d_x, amax=amax, g=g)


def gpu_weight_grads(pr, mode, fwd, bwd):
    """dW / db of every layer through the training step's own glue (autograd._weight_grads / _weight_grads_h); the
    layer-0 weight of the non-rigid MLP WITHOUT its condition-code columns (they are db x cond, see the callers)."""
    from humannerf_amd.autograd import _weight_grads, _weight_grads_h
    spec = SPECS[pr['kind']]
    if mode == 'f16x3h':
        return _weight_grads_h(bwd['dZ'], bwd['amax'], fwd['acts'], fwd['pe'], bwd['g'], fwd['ws'], skip_layer=spec['skip'],
                               skip_order=spec['order'], npe=spec['npe'])
    return _weight_grads(bwd['dZ'], fwd['acts'], fwd['pe'], bwd['g'], fwd['ws'], skip_layer=spec['skip'], skip_order=spec['order'],
                         amax=bwd['amax'], mode=mode)


def gpu_weight_grads_direct(pr, mode, fwd, bwd, fill):
    """The same calls as autograd._weight_grads / _weight_grads_h, made through the C ABI with output and workspace
    buffers of chosen contents."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    spec, P, half = SPECS[pr['kind']], pr['P'], mode == 'f16x3h'
    L, W, npe, n_head = spec['L'], spec['W'], spec['npe'], spec['n_out']
    st = torch.cuda.current_stream().cuda_stream
    dZ, acts, pe, g, amax = bwd['dZ'], fwd['acts'], fwd['pe'], bwd['g'], bwd['amax']
    gW = [_buf(tuple(w.shape), torch.float32, fill) for w in fwd['ws']]
    if pr['kind'] == 'nonrigid':
        gW[0] = _buf((W, npe), torch.float32, fill)
    gb = [_buf((w.shape[0],), torch.float32, fill) for w in fwd['ws']]

    def call(z, X, n_out, n_in, out, db, layout=0, scale=None, am=None):
        if half:
            need = lib.hnrf_mlp_dw_h_workspace_bytes(P, n_out, n_in)
            assert need > 0
            ws = _buf((need,), torch.uint8, fill)
            _lib.check(lib.hnrf_mlp_dw_h(z.data_ptr(), z.stride(0), X.data_ptr(), X.stride(0), P, n_out, n_in, layout,
                                         ops._ptr(scale), out.data_ptr(), out.stride(0), ops._ptr(db), ws.data_ptr(), ws.numel(), st),
                       'hnrf_mlp_dw_h')
        else:
            need = lib.hnrf_mlp_dw_workspace_bytes(P, n_out, n_in)
            assert need > 0
            ws = _buf((need,), torch.uint8, fill)
            use = mode if am is not None else 'f32'
            _lib.check(lib.hnrf_mlp_dw(z.data_ptr(), z.stride(0), X.data_ptr(), X.stride(0), P, n_out, n_in, ops.MLP_MODES[use],
                                       ops._ptr(am), 0 if am is None else am.numel(), out.data_ptr(), out.stride(0), ops._ptr(db),
                                       ws.data_ptr(), ws.numel(), st), 'hnrf_mlp_dw')
        torch.cuda.synchronize()

    ZB, XB = (1, 2) if half else (0, 0)
    call(g, acts[L - 1], n_head, W, gW[L], gb[L], layout=XB)
    for l in range(L):
        sc = amax[l:l + 1] if half else None
        am = None if half else amax[l]
        if l == 0:
            call(dZ[l], pe, W, npe, gW[l], gb[l], layout=ZB, scale=sc)
        elif l == spec['skip']:
            pe_cols = gW[l][:, :npe] if spec['order'] == 'pe_first' else gW[l][:, -npe:]
            h_cols = gW[l][:, npe:] if spec['order'] == 'pe_first' else gW[l][:, :-npe]
            call(dZ[l], pe, W, npe, pe_cols, None, layout=ZB, scale=sc)
            call(dZ[l], acts[l - 1], W, W, h_cols, gb[l], layout=ZB | XB, scale=sc, am=am)
        else:
            call(dZ[l], acts[l - 1], W, W, gW[l], gb[l], layout=ZB | XB, scale=sc, am=am)
    return gW, gb


def rows(m, P, half):
    """[L] (P, W) fp64 CPU matrices from an activation / dZ buffer of either layout"""
    return [_rows(m[l], P, half).double().cpu() for l in range(m.shape[0])]


def masks_of(fwd, P, half):
    return [(a > 0).double() for a in rows(fwd['acts'], P, half)]


def rel_errors(pr, ref, d_x, gW, gb, g=None):
    """{name: max error relative to the reference tensor's largest element}; a reference tensor that is identically
    zero (a dead ReLU row at P = 1) is compared absolutely: inf unless the result is exactly zero too."""
    def rel(a, b):
        a = a.double().cpu()
        if float(b.abs().max()) == 0.0:
            return 0.0 if float(a.abs().max()) == 0.0 else float('inf')
        return float((a - b).abs().max() / b.abs().max())
    n = len(gW)
    errs = {'d_x': rel(d_x, ref['d_x'])}
    for l in range(n):
        want = ref['dW'][l]
        if pr['kind'] == 'nonrigid' and l == 0:       # the caller's glue: condition-code columns = db x cond
            got = torch.cat([gb[0][:, None] * T(pr['cond']).reshape(1, -1), gW[0]], dim=1)
        else:
            got = gW[l]
        errs['W%d' % l] = rel(got, want)
        errs['b%d' % l] = rel(gb[l], ref['db'][l])
    return errs


def regime_of(kind):
    return 'scaled' if kind == 'nonrigid' else None


# ---------------------------------------------------------------------------------------------------------- A
def check_forward(pr, mode, fwd, label=''):
    spec, P, half = SPECS[pr['kind']], pr['P'], mode == 'f16x3h'
    with torch.no_grad():
        ref = ref_mlp(pr)
    out = fwd['out'].double().cpu()
    worst = {}
    if pr['kind'] == 'canonical':
        worst['raw'] = float((out - ref['out']).abs().max() / max(1.0, float(ref['out'].abs().max())))
        assert worst['raw'] <= 2e-5, worst
    else:
        worst['xyz'] = float((out - ref['out']).abs().max())
        worst['offsets'] = float((fwd['offsets'].double().cpu() - ref['offsets']).abs().max())
        assert worst['xyz'] <= 1e-5 and worst['offsets'] <= 1e-5, worst
    pe = fwd['pe'].double().cpu()
    npe = spec['npe']
    if half:
        assert fwd['pe'].dtype == torch.float16 and pe.shape == (P, 64)
        assert float(pe[:, npe:].abs().max()) == 0.0                       # padding columns: exactly zero
        e = (pe[:, :npe] - ref['pe']).abs() - (2.0 ** -11 * ref['pe'].abs() + 1e-6)
        worst['pe'] = float((pe[:, :npe] - ref['pe']).abs().max())
        assert float(e.max()) <= 0.0, float(e.max())
    else:
        assert pe.shape == (P, npe)
        worst['pe'] = float((pe - ref['pe']).abs().max())
        assert worst['pe'] <= 1e-6, worst
    acts = rows(fwd['acts'], P, half)
    assert fwd['acts'].dtype == (torch.float16 if half else torch.float32)
    for l in range(spec['L']):
        h = ref['acts'][l]
        bound = 2e-5 * max(1.0, float(h.abs().max()))
        err = (acts[l] - h).abs()
        worst['act%d' % l] = float(err.max() / max(1.0, float(h.abs().max())))
        if half:       # one f16 rounding on top: half an ulp, or half a subnormal step
            assert float((err - (bound + 2.0 ** -11 * h.abs() + 2.0 ** -25)).max()) <= 0.0, (l, worst)
        else:
            assert float(err.max()) <= bound, (l, worst)
        assert float(acts[l].min()) >= 0.0
    print('forward state', pr['kind'], mode, P, label, ' '.join('%s %.1e' % kv for kv in worst.items()))


@pytest.mark.parametrize('P', [1, 127, 128, 129, 256, 777, 4096])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind', KINDS)
def test_saved_forward_state_matches_fp64(kind, mode, P):
    """raw / xyz / offsets, the saved positional encoding and the saved activations of EVERY layer against fp64, for
    both MLPs in all three training modes.  P = 256 and 4096 in 'f16x3h' run the eight-wave non-rigid instance
    (nonrigid_f16x3_kernel<SV_ACT_H, 8>, the one the timed training step runs); every other case a four-wave one.
    Bounds: pe 1e-6 (f16: + 2^-11 |pe|, padding columns exactly 0), fp32 activations 2e-5 max(1, max|h|), f16-stored
    ones additionally one f16 rounding (2^-11 |h| + 2^-25, elementwise), xyz / offsets 1e-5."""
    pr = make_problem(kind, P, 1000 + P, regime_of(kind))
    check_forward(pr, mode, gpu_forward(pr, mode))


@pytest.mark.parametrize('P', [129, 256])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind', KINDS)
def test_saved_sign_masks_are_the_sign_of_the_saved_activations(kind, mode, P):
    """relu_bits is opaque; what it must encode is acts > 0.  The backward applies it: with an incoming gradient that is
    non-zero for every sample, dZ must be exactly zero where the saved activation is zero, and non-zero where it is
    positive (a live unit's dZ is a sum of 128 / 256 continuous random terms: it vanishes only by underflow, so at
    least 99.9 % of them must be non-zero; measured: all)."""
    pr = make_problem(kind, P, 2000 + P, regime_of(kind), dense_g=True)
    half = mode == 'f16x3h'
    fwd = gpu_forward(pr, mode)
    bwd = gpu_backward(pr, mode, fwd)
    live = masks_of(fwd, P, half)
    dZ = rows(bwd['dZ'], P, half)
    for l in range(SPECS[kind]['L']):
        assert 0.05 < float(live[l].mean()) < 0.95 or P == 1
        assert float((dZ[l] * (1 - live[l])).abs().max()) == 0.0, l
        nz = float(((dZ[l] != 0).double() * live[l]).sum() / live[l].sum())
        assert nz >= 0.999, (l, nz)


def test_eight_wave_nonrigid_forward_equals_four_wave_forward():
    """The eight-wave instance (P a multiple of 256) and the four-wave one are designed to agree bit for bit (same
    image, same per-wave arithmetic: csrc/hnrf_mlp_f16.hip at NR16W8_SLAB): P = 512 runs on the
    eight-wave form, the same samples with one appended (P = 513) on the four-wave form; the first 512 rows of every
    saved tensor are equal."""
    pr = make_problem('nonrigid', 513, 77, 'scaled')
    a = gpu_forward(pr, 'f16x3h')
    pr8 = dict(pr, P=512, x=pr['x'][:512], g=pr['g'][:512])
    b = gpu_forward(pr8, 'f16x3h')
    check_forward(pr8, 'f16x3h', b, label='(8 waves)')
    check_forward(pr, 'f16x3h', a, label='(4 waves)')
    assert torch.equal(a['out'][:512], b['out']) and torch.equal(a['offsets'][:512], b['offsets'])
    assert torch.equal(a['pe'][:512], b['pe']) and torch.equal(a['bits'][:, :512], b['bits'])
    for l in range(6):
        assert torch.equal(_rows(a['acts'][l], 512, True), _rows(b['acts'][l], 512, True)), l


# ------------------------------------------------------------------------------------------------------ B, C, E
def dw_from_saved_operands(pr, fwd, bwd):
    """fp64 dW / db from the f16 values the 'f16x3h' kernels saved: de-blocked activations, de-blocked dZ / scale."""
    spec, P = SPECS[pr['kind']], pr['P']
    scale = bwd['amax'].double().cpu()
    dZ = [z / scale[l] for l, z in enumerate(rows(bwd['dZ'], P, True))]
    return ref_weight_grads_from_operands(spec, dZ, rows(fwd['acts'], P, True), fwd['pe'].double().cpu()[:, :spec['npe']],
                                          bwd['g'].double().cpu())


def check_backward(pr, mode, g=None, amax_in=None, label='', fwd=None):
    """forward-train -> chain -> weight gradients against fp64 autograd with the kernel's sign pattern; in 'f16x3h'
    also against the fp64 product of the saved f16 operands.  Returns the errors."""
    spec, P, half = SPECS[pr['kind']], pr['P'], mode == 'f16x3h'
    fwd = gpu_forward(pr, mode) if fwd is None else fwd
    bwd = gpu_backward(pr, mode, fwd, g=g, amax_in=amax_in)
    gW, gb = gpu_weight_grads(pr, mode, fwd, bwd)
    ref = ref_mlp_grads(pr, masks_of(fwd, P, half), g)
    errs = rel_errors(pr, ref, bwd['d_x'], gW, gb)
    # dZ of every layer (fp32 modes: the stored values; 'f16x3h': after dividing the scale out, one f16 rounding)
    dZ = rows(bwd['dZ'], P, half)
    for l in range(spec['L']):
        want = ref['dZ'][l]
        got = dZ[l] / float(bwd['amax'][l]) if half else dZ[l]
        top = float(want.abs().max())
        errs['dZ%d' % l] = float((got - want).abs().max() / top) if top > 0 else (0.0 if float(got.abs().max()) == 0 else float('inf'))
    worst = max((v, k) for k, v in errs.items() if not k.startswith('dZ'))
    worst_z = max((v, k) for k, v in errs.items() if k.startswith('dZ'))
    print('backward', pr['kind'], mode, P, label, 'worst %.2e (%s) dZ %.2e (%s)' % (worst + worst_z), end=' ')
    if half:
        assert bwd['dZ'].dtype == torch.float16 and bwd['amax'].shape == (spec['L'],)
        sc = bwd['amax'].cpu()
        assert bool(torch.isfinite(sc).all()) and float(sc.min()) > 0
        assert all(float(torch.log2(a)) == round(float(torch.log2(a))) for a in sc)         # powers of two
        full = [_rows(bwd['dZ'][l], _pad128(P), True) for l in range(spec['L'])]
        assert all(float(f[P:].abs().max()) == 0.0 for f in full if f.shape[0] > P)            # padded rows: zeros
        oW, ob = dw_from_saved_operands(pr, fwd, bwd)
        for l in range(spec['L'] + 1):
            for name, got, want in (('W', gW[l], oW[l]), ('b', gb[l], ob[l])):
                top = float(want.abs().max())
                e = float((got.double().cpu() - want).abs().max() / top) if top > 0 else (0.0 if float(got.abs().max()) == 0 else float('inf'))
                errs['op_%s%d' % (name, l)] = e
        print('vs saved operands %.2e (%s)' % max((v, k) for k, v in errs.items() if k.startswith('op_')), end=' ')
    else:
        assert torch.equal(bwd['amax'].amax(1), bwd['dZ'].abs().amax(dim=(1, 2)))
    print()
    return errs, fwd, bwd


def assert_backward_bounds(errs, mode, label=''):
    """d_x 2e-5; dW / db 2e-5 (fp32 operands) or 1e-3 (f16 operands: two 11-bit roundings per product, see
    tests/test_gpu_grad.py::test_canonical_backward_chain_and_weight_gradients_match_autograd) of the tensor's largest
    element; f16 operands: 2e-6 against the fp64 product of the saved operands (hnrf_mlp_dw_h's own bound); dZ: 2e-5,
    with one f16 rounding (2^-11) on top where it is stored as f16."""
    half = mode == 'f16x3h'
    assert errs['d_x'] <= 2e-5, (label, 'd_x', errs['d_x'])
    for k, v in errs.items():
        if k.startswith('op_'):
            lim = 2e-6
        elif k.startswith('dZ'):
            lim = 2e-5 + (2.0 ** -11 if half else 0.0)
        else:
            lim = 1e-3 if half else 2e-5
        assert v <= lim, (label, k, v, errs)


@pytest.mark.parametrize('regime', ['scaled', 'fresh_init'])
def test_nonrigid_backward_chain_and_weight_gradients_f16_operands(regime):
    """tests/test_gpu_grad.py::test_nonrigid_backward_chain_and_weight_gradients_match_autograd in 'f16x3h', the default
    training arithmetic: nonrigid_f16x3_kernel<SV_ACT_H>, nonrigid_bwd16_kernel<true>, the 128-wide blocked layout and
    the hand-off of those buffers to hnrf_mlp_dw_h (scale, padded rows, the PE matrix with 36 real columns).  Same
    inputs (P = 1000), d_x_skel 2e-5, every dW / db 1e-3 of its own largest element against fp64 autograd and 2e-6
    against the fp64 product of the f16 operands the kernels saved."""
    from humannerf_amd.autograd import OperandRangeGuard
    pr = make_problem('nonrigid', 1000, 12, regime)
    errs, fwd, bwd = check_backward(pr, 'f16x3h', label=regime)
    flags = [bool(f) for f in OperandRangeGuard.flags([fwd['acts']], bwd['g'], [bwd['dZ']])]
    assert flags == [False, False, False]
    assert_backward_bounds(errs, 'f16x3h', regime)


def test_canonical_weight_gradients_equal_product_of_saved_f16_operands():
    """The canonical MLP at the existing chain test's size (P = 777): every dW / db of 'f16x3h' is the fp64 product of
    the saved f16 operands to 2e-6 -- the kernel separated from the operands' rounding."""
    pr = make_problem('canonical', 777, 11)
    errs, _, _ = check_backward(pr, 'f16x3h')
    assert_backward_bounds(errs, 'f16x3h')


def test_range_guard_flags_tiny_hidden_layer_in_f16_operand_mode():
    """``tiny_hidden`` (a layer of 1e-6 activations) is outside the premise of the f16-operand arithmetic: it is not
    held to the bounds there, the guard must flag it (first flag), and only it."""
    from humannerf_amd.autograd import OperandRangeGuard
    pr = make_problem('nonrigid', 1000, 12, 'tiny_hidden')
    fwd = gpu_forward(pr, 'f16x3h')
    bwd = gpu_backward(pr, 'f16x3h', fwd)
    flags = [bool(f) for f in OperandRangeGuard.flags([fwd['acts']], bwd['g'], [bwd['dZ']])]
    assert flags == [True, False, False]
    for regime in ('scaled', 'fresh_init'):
        q = make_problem('nonrigid', 1000, 12, regime)
        f = gpu_forward(q, 'f16x3h')
        assert [bool(x) for x in OperandRangeGuard.flags([f['acts']], T(q['g']))] == [False, False, False]


@pytest.mark.parametrize('P', [1, 127, 128, 129, 256, 4096])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind', KINDS)
def test_backward_chain_and_weight_gradients_across_sample_counts(kind, mode, P):
    """Both chains and every weight gradient at one sample, around the 128-sample workgroup (127 / 128 / 129), at whole
    256-sample workgroups (the eight-wave forward) and at 4096, in all three modes; tolerances as at the existing sizes."""
    pr = make_problem(kind, P, 3000 + P, regime_of(kind))
    errs, _, _ = check_backward(pr, mode)
    assert_backward_bounds(errs, mode)


@pytest.mark.parametrize('kind', KINDS)
def test_backward_chain_and_weight_gradients_at_66048_samples(kind):
    """P = 66 048 = 258 x 256 in 'f16x3h': another slice plan of the weight-gradient kernels than P = 4096, the
    eight-wave forward, 516 workgroups of the chains."""
    pr = make_problem(kind, 66048, 4000, regime_of(kind))
    errs, _, _ = check_backward(pr, 'f16x3h')
    assert_backward_bounds(errs, 'f16x3h')


@pytest.mark.parametrize('slack', [1.0, 1000.0])
@pytest.mark.parametrize('gscale', [2.0 ** -24, 1.0, 2.0 ** 10])
@pytest.mark.parametrize('mode', ['f16x3', 'f16x3h'])
@pytest.mark.parametrize('kind', KINDS)
def test_backward_is_independent_of_the_gradient_scale(kind, mode, gscale, slack):
    """The incoming gradient multiplied by 2^-24 (a real loss gradient's size), 1 and 2^10: the fp64 reference scales
    exactly, the same relative bounds hold (measured: the errors are the SAME numbers at all three sizes).  slack = 1000:
    the amax argument is a loose bound (1000 x the true maximum, not a power of two), which include/hnrf.h allows and
    states the price of: ten bits of the range below the largest value.  Measured: 'f16x3' 6.9e-7 -> 7.5e-7 (canonical),
    5.2e-7 -> 1.0e-6 (non-rigid); 'f16x3h' worst dW / db 3.5e-4 -> 3.6e-4 (canonical), 4.6e-4 -> 9.0e-4 (non-rigid, b0):
    inside the 1e-3 bound, which is why the header says to keep the bound within that factor."""
    pr = make_problem(kind, 777, 5000, regime_of(kind))
    g = pr['g'] * np.float32(gscale)
    amax_in = None if slack == 1.0 else float(np.abs(g).max()) * slack
    errs, _, _ = check_backward(pr, mode, g=g, amax_in=amax_in, label='g x %g amax x %g' % (gscale, slack))
    assert_backward_bounds(errs, mode, (gscale, slack))


@pytest.mark.parametrize('mode', ['f16x3', 'f16x3h'])
@pytest.mark.parametrize('kind', KINDS)
def test_zero_incoming_gradient_gives_exact_zeros(kind, mode):
    """Every ray of a batch misses the body, or T-pose frames: the incoming gradient and its amax are zero.  Every
    output is finite and exactly zero; the non-rigid d_x_skel is the incoming d_xyz bit for bit (identity path) -- also
    for a non-zero d_xyz whose MLP path is cut (checked with zero head weights); the scales are finite and positive."""
    pr = make_problem(kind, 777, 6000, regime_of(kind))
    half = mode == 'f16x3h'
    fwd = gpu_forward(pr, mode)
    bwd = gpu_backward(pr, mode, fwd, g=pr['g'] * 0)
    gW, gb = gpu_weight_grads(pr, mode, fwd, bwd)
    for t in [bwd['dZ'], bwd['d_x']] + list(gW) + list(gb):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0
    assert bool(torch.isfinite(bwd['amax']).all())
    if half:
        assert float(bwd['amax'].min()) > 0
    else:
        assert float(bwd['amax'].abs().max()) == 0.0
    if kind == 'nonrigid':
        q = dict(pr, ws=pr['ws'][:-1] + [pr['ws'][-1] * 0])
        f = gpu_forward(q, mode)
        b = gpu_backward(q, mode, f)
        assert torch.equal(b['d_x'], b['g'])


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('mode', ['f16x3', 'f16x3h'])
@pytest.mark.parametrize('kind', KINDS)
def test_non_finite_incoming_gradient_is_visible_in_every_output(kind, mode, bad):
    """One inf / NaN in the incoming gradient (an overflowed loss): the scale is undefined and the kernels are
    documented to return NaN everywhere so that the caller's finite check sees it.  What that check relies on: d_x
    and the dW / db of every layer fail isfinite().all().  (In 'f16x3' the matrix-shaped dW came out FINITE before
    hnrf_*_bwd initialised dz_amax to NaN for a non-finite bound: the weight-gradient kernel clamps its operands.)"""
    pr = make_problem(kind, 777, 7000, regime_of(kind))
    g = pr['g'].copy()
    g[388, 1] = bad
    fwd = gpu_forward(pr, mode)
    bwd = gpu_backward(pr, mode, fwd, g=g)
    gW, gb = gpu_weight_grads(pr, mode, fwd, bwd)
    assert not bool(torch.isfinite(bwd['d_x']).all())
    for l, (w, b) in enumerate(zip(gW, gb)):
        assert not bool(torch.isfinite(w).all()), ('dW', l)
        assert not bool(torch.isfinite(b).all()), ('db', l)


# ---------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize('P', [777, 1])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind', KINDS)
def test_results_do_not_depend_on_previous_buffer_contents(kind, mode, P):
    """forward-train -> chain -> every weight-gradient call, once into zero-filled output and workspace buffers and once
    into poisoned ones (f16 NaN 0x7E00, fp32 NaN, 0xFFFFFFFF in relu_bits), as the caching allocator hands them out in a
    training loop: every result is finite, the real rows are bit-identical, and in 'f16x3h' the padded rows of the
    blocked dZ are exactly zero whatever was there before (the weight-gradient kernel reads whole blocks)."""
    pr = make_problem(kind, P, 8000 + P, regime_of(kind))
    spec, half = SPECS[kind], mode == 'f16x3h'
    runs = {}
    for fill in ('zero', 'poison'):
        fwd = gpu_forward(pr, mode, fill)
        bwd = gpu_backward(pr, mode, fwd, fill=fill)
        gW, gb = gpu_weight_grads_direct(pr, mode, fwd, bwd, fill)
        runs[fill] = (fwd, bwd, gW, gb)
    (f0, b0, W0, B0), (f1, b1, W1, B1) = runs['zero'], runs['poison']
    for name in ('out', 'offsets', 'pe', 'bits'):
        if f0[name] is not None:
            assert torch.equal(f0[name], f1[name]), name
            assert f0[name].dtype == torch.int32 or bool(torch.isfinite(f1[name]).all()), name
    for l in range(spec['L']):
        for name, a, b in (('acts', f0['acts'][l], f1['acts'][l]), ('dZ', b0['dZ'][l], b1['dZ'][l])):
            ra, rb = _rows(a, P, half), _rows(b, P, half)
            assert bool(torch.isfinite(rb).all()) and torch.equal(ra, rb), (name, l)
        if half:
            pad = _rows(b1['dZ'][l], _pad128(P), True)[P:]
            assert pad.shape[0] == _pad128(P) - P and float(pad.abs().max()) == 0.0, l
            full = _rows(f1['acts'][l], _pad128(P), True)                                   # padded activation rows: row P-1
            assert bool(torch.isfinite(full).all()) and torch.equal(full[P:], full[P - 1:P].expand(_pad128(P) - P, -1)), l
    assert torch.equal(b0['d_x'], b1['d_x']) and bool(torch.isfinite(b1['d_x']).all())
    assert torch.equal(b0['amax'], b1['amax']) and bool(torch.isfinite(b1['amax']).all())
    for l in range(spec['L'] + 1):
        assert bool(torch.isfinite(W1[l]).all()) and bool(torch.isfinite(B1[l]).all()), l
        assert torch.equal(W0[l], W1[l]) and torch.equal(B0[l], B1[l]), l
    # and the direct calls are the calls of the training step's glue
    gW, gb = gpu_weight_grads(pr, mode, f0, b0)
    for l in range(spec['L'] + 1):
        assert torch.equal(gW[l], W0[l]) and torch.equal(gb[l], B0[l]), l


# ---------------------------------------------------------------------------------------------------------- F
COMPOSITE_S = [2, 50, 64, 100, 128, 256, 300, 512]


@pytest.mark.parametrize('regime', ['sparse', 'dense', 'opaque'])
@pytest.mark.parametrize('S', COMPOSITE_S)
@pytest.mark.parametrize('R', [1, 19, 1030])
def test_composite_bwd_kernel_shapes(R, S, regime):
    """hnrf_composite_bwd against fp64 autograd of oracle.raw2outputs for every samples-per-lane instance (S = 2 ..
    512), a ragged last lane (50, 100, 300), one ray / a ragged last workgroup (R = 1, 19, 1030), with all three upstream
    gradients and with g_alpha = g_depth = None.  'sparse' (the existing inputs): 2e-5 of max(1, max|ref|).  'dense' /
    'opaque' (the transmittance collapses inside the ray; opaque: 1 - alpha + 1e-10 is the 1e-10 floor): 4 x the distance
    of the oracle's own fp32 autograd from fp64, but not less than 2e-5.  Measured over all cases (MI355X): fp32 floor
    <= 1.9e-7 (d_raw), <= 3.8e-7 (d_mask), so 2e-5 governs everywhere; the kernel's error <= 2.2e-7 (d_raw), <= 3.6e-7
    (d_mask; sparse 5.1e-7); each case's two numbers are printed.  Before the exclusive suffix sum over lanes was taken
    from the next lane (csrc/hnrf_backward.hip) d_mask was wrong by up to 1.8 x its largest element in the dense regimes
    and by 3e-5 .. 2e-4 in the sparse one at R = 1030: these cases found it."""
    from humannerf_amd import ops
    c = composite_problem(R, S, regime, seed=5 + S)
    names = ['raw', 'mask', 'z', 'rays_d', 'bg', 'g_rgb']
    for with_ad in (True, False):
        extra = (T(c['g_a']), T(c['g_d'])) if with_ad else (None, None)
        d_raw, d_mask = ops.composite_bwd(*[T(c[n]) for n in names], *extra)
        ref = ref_composite_grads(c, torch.float64, with_ad)
        if regime == 'sparse':
            floor = (0.0, 0.0)
        else:
            f32 = ref_composite_grads(c, torch.float32, with_ad)
            floor = tuple(float((a.double() - b).abs().max() / max(1.0, float(b.abs().max()))) for a, b in zip(f32, ref))
        for name, got, want, fl in (('d_raw', d_raw, ref[0], floor[0]), ('d_mask', d_mask, ref[1], floor[1])):
            assert bool(torch.isfinite(got).all()), name
            err = float((got.cpu().double() - want).abs().max() / max(1.0, float(want.abs().max())))
            print('composite bwd', R, S, regime, 'a/d' if with_ad else 'rgb only', name, 'err %.2e fp32 floor %.2e' % (err, fl))
            assert err <= max(2e-5, 4 * fl), (name, err, fl)


def test_composite_bwd_refuses_more_than_512_samples():
    from humannerf_amd import _lib, ops
    c = composite_problem(3, 513, 'sparse')
    with pytest.raises(_lib.HnrfError, match=r'\(-2\)'):                   # HNRF_E_UNSUPPORTED, nothing launched
        ops.composite_bwd(*[T(c[n]) for n in ('raw', 'mask', 'z', 'rays_d', 'bg', 'g_rgb')])
    torch.cuda.synchronize()


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('P', [1, 255, 256, 257, 777])
def test_pe_bwd_kernel_shapes(P, accumulate):
    """hnrf_pe_bwd for both encoders around its 256-thread block, writing and accumulating: with accumulate the result
    is the previous contents + the fp64 gradient, to the existing 1e-4 of the gradient's largest element."""
    from humannerf_amd import ops
    rs = np.random.RandomState(40 + P)
    x = rs.uniform(-1.2, 1.2, (P, 3)).astype(np.float32)
    for nb, inc, hw in ((10, True, None), (6, False, np.array([1, 1, 0.7, 0.2, 0, 0], dtype=np.float32))):
        C = (3 if inc else 0) + 6 * nb
        g = rs.randn(P, C).astype(np.float32)
        ref = ref_pe_grad(x, g, nb, hw)
        pre = (rs.randn(P, 3) * float(ref.abs().max())).astype(np.float32)
        out = T(pre) if accumulate else None
        got = ops.pe_bwd(T(x), T(g), None if hw is None else T(hw), nb, inc, out=out)
        want = ref + (torch.from_numpy(pre).double() if accumulate else 0.0)
        err = float((got.cpu().double() - want).abs().max() / ref.abs().max())
        assert err <= 1e-4, (nb, err)
