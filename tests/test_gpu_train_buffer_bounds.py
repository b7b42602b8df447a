"""Where the training kernels write and read: the "training (backward)" entries of include/hnrf.h, those of
include/hnrf_heads_train.h and hnrf_deconv_fold, under the five assertions of tests/test_gpu_buffer_bounds.py.  Every
input, output, packed image, saved buffer and workspace of every call sits in a guarded buffer (tests/guarded_buffers.py)
of EXACTLY the size the header states or the ``*_bytes`` function returns, the call runs once under each of the two
fills, and

  (a) every guard is intact,
  (b) every output is bit-equal between the two fills,
  (c) every output is bit-equal to the same call through the ops wrapper on allocator-provided buffers,
  (d) what the contract calls unwritten still holds the fill (the columns of dW outside the block, the tail of
      d_x_parts), what it calls padding holds what it says (zero columns of pe_out, copies of row P-1 in blocked acts,
      zero rows in blocked dZ), and a refused call or a P == 0 call leaves everything at the fill,
  (e) every input holds what it held.

The guards are 256 KiB here: one 128-sample tile of a 256-wide fp32 layer is 128 KiB, so a kernel that writes one whole
padding tile too many still lands inside the guard (tests/test_guarded_buffers_cpu.py plants that store).  Every
comparison is on bit patterns, with one exception: the outputs of hnrf_sample_warp_bwd are sums of float atomics, so
(b) and (c) become "each run is finite and within tests/test_warp_bwd_refs.py's own bound of the fp64 reference"
(wrefs.errors: 4 x the error of the reference's fp32 evaluation) -- a NaN fill that leaks in fails the first.  The
values themselves are checked elsewhere (tests/test_gpu_train_kernels.py and the files beside it); the problems are
theirs.  P = 777 = 37 x 21 unless a test says otherwise.  The C entries are called through humannerf_amd._lib with raw
pointers.  Needs an MI355X: ``pytest -m gpu``."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import guarded_buffers as gb
from tests import test_warp_bwd_refs as wrefs
from tests.guarded_case import Case, T, _stream, bits, dev, ok, same
from tests.heads_train_cases import make_heads_problem
from tests.test_train_kernel_refs import SPECS, composite_problem, make_problem

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 256 * 1024
R0, S0 = 37, 21
P0 = R0 * S0
E_ARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4
MODES = ['f32', 'f16x3', 'f16x3h']
PACK_MODES = ['f32', 'f16x3']
# 1: one sample; 128: the blocked layers have no padding rows; 256: the non-rigid forward's eight-wave form
SAMPLE_COUNTS = [P0, 1, 128, 256]
NETS = [('canonical', 0), ('nonrigid', 0), ('canonical', 2), ('canonical', 3), ('canonical', 8)]
NET_IDS = ['canonical', 'nonrigid', 'heads2', 'heads3', 'heads8']
SEED = 4100
AMAX_SLOTS = 64


def both(fn):
    """fn(case) under each fill, 256 KiB guards -> the two finished cases."""
    out = []
    for fill in gb.FILLS:
        c = Case(fill, GUARD)
        fn(c)
        out.append(c.done())
    return out


def lib_train():
    from humannerf_amd import _lib
    return _lib.load_heads_train()


def as_bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def eqb(c, name, t, nbytes=None):
    """(c): the interior of buffer ``name`` holds the bytes of tensor ``t`` (its first ``nbytes``)."""
    want = as_bytes(t)
    want = want if nbytes is None else want[:nbytes]
    got = c.g[name].interior_bytes()
    assert got.numel() == want.numel() and torch.equal(got, want), name


def pad128(P):
    return (P + 127) // 128 * 128


def unblock(m):
    """[P128, W] of one blocked layer -> its rows in sample order."""
    from tests.test_gpu_grad import _rows
    return _rows(m, m.shape[0], True)


def to_blocked(m):
    from tests.test_gpu_grad import _to_blocked
    return _to_blocked(m)


# ================================================================================================ the two MLPs and the heads
@functools.lru_cache(maxsize=None)
def mlp_problem(kind, H, P):
    """The weights are those of the seed, whatever P is: one packed image per network serves every sample count."""
    if H:
        return make_heads_problem(H, P, SEED)
    return make_problem(kind, P, SEED, 'scaled' if kind == 'nonrigid' else None)


@functools.lru_cache(maxsize=None)
def dev_weights(kind, H):
    pr = mlp_problem(kind, H, P0)
    for P in SAMPLE_COUNTS[1:] + [0]:
        assert all(np.array_equal(a, b) for a, b in zip(pr['ws'] + pr['bs'], mlp_problem(kind, H, P)['ws'] + mlp_problem(kind, H, P)['bs']))
    return [T(w) for w in pr['ws']], [T(b) for b in pr['bs']]


@functools.lru_cache(maxsize=None)
def fwd_image(kind, H, pm):
    """(tensor, exact bytes, status offset) of the forward image in pack mode ``pm``."""
    from humannerf_amd import ops
    lib = lib_train()
    ws, bs = dev_weights(kind, H)
    m = ops.MLP_MODES[pm]
    if kind == 'nonrigid':
        t = ops.nonrigid_pack(ws, bs, T(mlp_problem(kind, H, P0)['cond']), pm)
        nbytes, off = lib.hnrf_nonrigid_packed_bytes(m), lib.hnrf_nonrigid_status_offset(m)
    else:
        t = ops.canonical_heads_pack(ws, bs, H, pm) if H else ops.canonical_pack(ws, bs, pm)
        nbytes, off = lib.hnrf_canonical_packed_bytes(m), lib.hnrf_canonical_status_offset(m)
    torch.cuda.synchronize()
    assert 0 < nbytes <= t.numel() * 4 and off + 4 <= nbytes and off % 4 == 0
    return t, nbytes, off


def bwd_packed_bytes(lib, kind, H, pm):
    from humannerf_amd import ops
    m = ops.MLP_MODES[pm]
    if H:
        return lib.hnrf_canonical_heads_bwd_packed_bytes(m, H)
    return (lib.hnrf_canonical_bwd_packed_bytes if kind == 'canonical' else lib.hnrf_nonrigid_bwd_packed_bytes)(m)


@functools.lru_cache(maxsize=None)
def bwd_image(kind, H, pm):
    """(tensor of the pack wrapper, exact bytes) of the transposed image."""
    from humannerf_amd import ops
    ws, _ = dev_weights(kind, H)
    if H:
        t = ops.canonical_heads_bwd_pack(ws, H, pm)
    else:
        t = (ops.canonical_bwd_pack if kind == 'canonical' else ops.nonrigid_bwd_pack)(ws, pm)
    torch.cuda.synchronize()
    nbytes = bwd_packed_bytes(lib_train(), kind, H, pm)
    assert 0 < nbytes <= t.numel() * 4
    return t, nbytes


def saved_bytes(kind, P, mode):
    """Bytes of pe_out, acts (= dZ) and relu_bits as the header states them."""
    spec, half = SPECS[kind], mode == 'f16x3h'
    L, W = spec['L'], spec['W']
    return dict(pe=P * 64 * 2 if half else P * spec['npe'] * 4, acts=L * pad128(P) * W * 2 if half else L * P * W * 4,
                bits=L * P * spec['nb'] * 4)


@functools.lru_cache(maxsize=None)
def fwd_ops(kind, H, P, mode):
    """The forward through the ops wrapper on allocator buffers: dict of its outputs (the backward's inputs too)."""
    from humannerf_amd import ops
    pr = mlp_problem(kind, H, P)
    image = fwd_image(kind, H, 'f16x3' if mode == 'f16x3h' else mode)[0].clone()
    if kind == 'nonrigid':
        out = dict(zip(('xyz', 'offsets', 'pe', 'acts', 'bits'), ops.nonrigid_train(T(pr['x']), T(pr['hann']), image, mode)))
    elif H:
        out = dict(zip(('raw', 'pe', 'acts', 'bits'), ops.canonical_heads_train(T(pr['x']), image, H, mode)))
    else:
        out = dict(zip(('raw', 'pe', 'acts', 'bits'), ops.canonical_train(T(pr['x']), image, mode)))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('P', SAMPLE_COUNTS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind,H', NETS, ids=NET_IDS)
def test_forward_train(kind, H, mode, P):
    """hnrf_canonical_fwd_train, hnrf_nonrigid_fwd_train, hnrf_canonical_heads_fwd_train: f16x3h writes pe_out as f16
    [P][64] and acts as f16 [L][ceil(P / 128) * 128][W], the other modes fp32 [P][63 | 36] and [L][P][W]; relu_bits is
    [L][P][8 | 4] uint32.  The padding contract: padding columns of pe_out are zero, padding rows of every blocked acts
    layer equal row P - 1, under both fills."""
    from humannerf_amd import ops
    lib = lib_train()
    spec, half = SPECS[kind], mode == 'f16x3h'
    pr, sz = mlp_problem(kind, H, P), saved_bytes(kind, P, mode)
    image = fwd_image(kind, H, 'f16x3' if half else mode)
    m = ops.TRAIN_MODES[mode]
    names = (['xyz', 'offsets'] if kind == 'nonrigid' else ['raw']) + ['pe', 'acts', 'bits']

    def call(c):
        x, img = c.put('x', pr['x']), c.packed('image', image)
        saved = [c.new('pe', sz['pe']), c.new('acts', sz['acts']), c.new('bits', sz['bits'])]
        if kind == 'nonrigid':
            ok(lib.hnrf_nonrigid_fwd_train(x, c.put('hann', pr['hann']), img, m, P, c.new('xyz', 12 * P), c.new('offsets', 12 * P),
                                           *saved, _stream()), 'hnrf_nonrigid_fwd_train')
        elif H:
            ok(lib.hnrf_canonical_heads_fwd_train(x, img, m, P, H, c.new('raw', 16 * P * H), *saved, _stream()),
               'hnrf_canonical_heads_fwd_train')
        else:
            ok(lib.hnrf_canonical_fwd_train(x, img, m, P, c.new('raw', 16 * P), *saved, _stream()), 'hnrf_canonical_fwd_train')
    a, b = both(call)
    same(a, b, names)
    want = fwd_ops(kind, H, P, mode)
    for n in names:
        eqb(a, n, want[n])
    if half:
        L, W, P128 = spec['L'], spec['W'], pad128(P)
        for c in (a, b):
            pe = c.g['pe'].view(torch.float16, P, 64)
            assert bool((pe[:, spec['npe']:].view(torch.int16) == 0).all())
            acts = c.g['acts'].view(torch.float16, L, P128, W)
            for l in range(L):
                full = unblock(acts[l])
                assert torch.equal(full[P:].view(torch.int16), full[P - 1:P].expand(P128 - P, W).view(torch.int16)), l


@pytest.mark.parametrize('kind,H', NETS, ids=NET_IDS)
def test_forward_train_without_samples(kind, H):
    """P == 0: HNRF_OK and nothing is written (every output has zero bytes: the guards see a store)."""
    from humannerf_amd import ops
    lib = lib_train()
    pr = mlp_problem(kind, H, P0)
    for mode in MODES:
        image = fwd_image(kind, H, 'f16x3' if mode == 'f16x3h' else mode)
        m = ops.TRAIN_MODES[mode]

        def call(c):
            x, img = c.new('x', 0), c.packed('image', image)
            saved = [c.new('pe', 0), c.new('acts', 0), c.new('bits', 0)]
            if kind == 'nonrigid':
                ok(lib.hnrf_nonrigid_fwd_train(x, c.put('hann', pr['hann']), img, m, 0, c.new('xyz', 0), c.new('offsets', 0),
                                               *saved, _stream()), 'hnrf_nonrigid_fwd_train')
            elif H:
                ok(lib.hnrf_canonical_heads_fwd_train(x, img, m, 0, H, c.new('raw', 0), *saved, _stream()),
                   'hnrf_canonical_heads_fwd_train')
            else:
                ok(lib.hnrf_canonical_fwd_train(x, img, m, 0, c.new('raw', 0), *saved, _stream()), 'hnrf_canonical_fwd_train')
        both(call)


@pytest.mark.parametrize('pm', PACK_MODES)
@pytest.mark.parametrize('kind,H', NETS, ids=NET_IDS)
def test_backward_pack(kind, H, pm):
    """hnrf_canonical_bwd_pack, hnrf_nonrigid_bwd_pack, hnrf_canonical_heads_bwd_pack: the image is exactly
    *_bwd_packed_bytes(mode[, n_heads]) bytes and every byte of it is written; each weight matrix sits in a buffer of
    exactly out x in floats."""
    from humannerf_amd import ops
    lib = lib_train()
    pr = mlp_problem(kind, H, P0)
    nbytes = bwd_packed_bytes(lib, kind, H, pm)
    assert nbytes > 0
    m = ops.MLP_MODES[pm]

    def call(c):
        ptrs = (ctypes.c_void_p * len(pr['ws']))(*[c.put('w%d' % l, w) for l, w in enumerate(pr['ws'])])
        if H:
            ok(lib.hnrf_canonical_heads_bwd_pack(ptrs, H, m, c.new('image', nbytes), _stream()), 'hnrf_canonical_heads_bwd_pack')
        else:
            fn = lib.hnrf_canonical_bwd_pack if kind == 'canonical' else lib.hnrf_nonrigid_bwd_pack
            ok(fn(ptrs, m, c.new('image', nbytes), _stream()), 'hnrf_%s_bwd_pack' % kind)
    a, b = both(call)
    same(a, b, ['image'])
    eqb(a, 'image', bwd_image(kind, H, pm)[0], nbytes)
    if H:                                                        # no image of its own: zero bytes
        assert lib.hnrf_canonical_heads_bwd_packed_bytes(2, H) == 0 and lib.hnrf_canonical_heads_bwd_packed_bytes(m, 9) == 0


def bwd_call(lib, c, kind, H, P, mode, pr, fwd_bits, want_amax):
    """One call of a chain entry with every buffer in ``c``; returns the names of its outputs."""
    from humannerf_amd import ops
    spec, half = SPECS[kind], mode == 'f16x3h'
    sz = saved_bytes(kind, P, mode)
    t, nbytes = bwd_image(kind, H, 'f16x3' if half else mode)
    g = pr['g']
    x = c.put('x', pr['x']) if P else c.new('x', 0)
    gp = c.put('g', g) if P else c.new('g', 0)
    rb = c.put('bits', fwd_bits) if P else c.new('bits', 0)
    img = c.put('image', t.view(torch.uint8)[:nbytes].clone())
    am = None if mode == 'f32' else c.put('g_amax', np.array([np.abs(g).max() if P else 1.0], F))
    dZ, dx = c.new('dZ', sz['acts']), c.new('d_x', 12 * P)
    amax = c.new('dz_amax', 4 * spec['L'] * (1 if half else AMAX_SLOTS)) if want_amax else None
    m = ops.TRAIN_MODES[mode]
    if kind == 'nonrigid':
        ok(lib.hnrf_nonrigid_bwd(x, c.put('hann', pr['hann']), gp, rb, img, m, am, P, dZ, dx, amax, _stream()), 'hnrf_nonrigid_bwd')
    elif H:
        ok(lib.hnrf_canonical_heads_bwd(x, gp, rb, img, m, am, P, H, dZ, dx, amax, _stream()), 'hnrf_canonical_heads_bwd')
    else:
        ok(lib.hnrf_canonical_bwd(x, gp, rb, img, m, am, P, dZ, dx, amax, _stream()), 'hnrf_canonical_bwd')
    return ['dZ', 'd_x'] + (['dz_amax'] if want_amax else [])


@pytest.mark.parametrize('P', SAMPLE_COUNTS)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind,H', NETS, ids=NET_IDS)
def test_backward_chain(kind, H, mode, P):
    """hnrf_canonical_bwd, hnrf_nonrigid_bwd, hnrf_canonical_heads_bwd: dZ is sized like acts, d_xyz / d_x_skel is [P,3],
    dz_amax is [L][HNRF_AMAX_SLOTS] (given and NULL) in the fp32-dZ modes and [L] in f16x3h, the bound of the incoming
    gradient a one-float buffer, d_raw of the heads [H][P][4].  In f16x3h the padding rows of blocked dZ are zero under
    both fills."""
    from humannerf_amd import ops
    lib = lib_train()
    spec, half = SPECS[kind], mode == 'f16x3h'
    pr, fwd = mlp_problem(kind, H, P), fwd_ops(kind, H, P, mode)
    ws, _ = dev_weights(kind, H)
    if kind == 'nonrigid':
        want = ops.nonrigid_bwd(T(pr['x']), T(pr['hann']), T(pr['g']), fwd['bits'], ws, mode)
    elif H:
        want = ops.canonical_heads_bwd(T(pr['x']), T(pr['g']), fwd['bits'], ws, H, mode)
    else:
        want = ops.canonical_bwd(T(pr['x']), T(pr['g']), fwd['bits'], ws, mode)
    torch.cuda.synchronize()
    want = dict(zip(('dZ', 'd_x', 'dz_amax'), want))
    for want_amax in ([True] if half else [True, False]):
        names = []
        a, b = both(lambda c: names.append(bwd_call(lib, c, kind, H, P, mode, pr, fwd['bits'], want_amax)))
        same(a, b, names[0])
        for n in names[0]:
            eqb(a, n, want[n])
        if half:
            L, W, P128 = spec['L'], spec['W'], pad128(P)
            for c in (a, b):
                dZ = c.g['dZ'].view(torch.float16, L, P128, W)
                for l in range(L):
                    assert bool((unblock(dZ[l])[P:] == 0).all()), l


@pytest.mark.parametrize('kind,H', NETS, ids=NET_IDS)
def test_backward_chain_without_samples(kind, H):
    """P == 0 returns HNRF_OK with everything at the fill, dz_amax included."""
    lib = lib_train()
    pr = mlp_problem(kind, H, 0)
    for mode in MODES:
        for c in both(lambda c: bwd_call(lib, c, kind, H, 0, mode, pr, None, True)):
            for n in ('dZ', 'd_x', 'dz_amax'):
                c.g[n].holds_fill()


# ================================================================================================ the weight gradients
# (n_out, n_in) -> (ldw, first column) of its block in the gradient it is written into: the two blocks of the canonical
# skip layer's (256, 319) weight, PE first; the two of the non-rigid one's (128, 164), PE last; the others whole.
DW_SHAPES = {(256, 256): (319, 63), (256, 63): (319, 0), (128, 128): (164, 0), (128, 36): (164, 128), (256, 128): (128, 0),
             (4, 256): (256, 0), (3, 128): (128, 0)}
DW_IDS = ['%dx%d' % s for s in DW_SHAPES]


def matrix_shaped(n_out, n_in):
    return n_out > 4 and n_in > 64


@functools.lru_cache(maxsize=None)
def dw_operands(P, n_out, n_in):
    rs = np.random.RandomState(11 * P + n_out + 3 * n_in)
    return rs.standard_normal((P, n_out)).astype(F), np.maximum(rs.standard_normal((P, n_in)), 0).astype(F)


def tight(m, ld):
    """[P, width] -> the (P - 1) * ld + width elements of the same matrix at row stride ld, NaN between the rows."""
    P, w = m.shape
    buf = torch.full((P, ld), float('nan'), dtype=m.dtype, device=m.device)
    buf[:, :w] = m
    return buf.reshape(-1)[:(P - 1) * ld + w].clone()


def strided(flat, P, ld, width):
    """The [P, width] view at row stride ld of what ``tight`` made (for the ops wrapper)."""
    return torch.as_strided(flat, (P, width), (ld, 1))


def block_columns(n_out, n_in, ldw):
    """Boolean mask over the tight dW buffer's (n_out - 1) * ldw + n_in floats: True where the block lies."""
    k = torch.arange((n_out - 1) * ldw + n_in, device=dev())
    return k % ldw < n_in


def other_call(need, P, shape):
    """Another (P, shape) whose workspace fits into that of (P, shape): first of a fixed list."""
    have = need(P, *shape)
    for cand in [(q,) + s for q in (300, 5) for s in DW_SHAPES] + [(200, 3, 128), (3, 3, 128)]:
        if cand != (P,) + shape and 0 < need(*cand) <= have:
            return cand[0], cand[1:]
    raise AssertionError('no other call fits the workspace of %r' % ((P,) + shape,))


class DwCall:
    """One call of hnrf_mlp_dw (``entry`` 'f32' | 'f16x3') or hnrf_mlp_dw_h ('h0' | 'h1' | 'h2' | 'h3': the layout) on
    dw_operands(P, n_out, n_in): ``run`` makes it with every buffer in a case, ``ops`` through the wrapper."""

    def __init__(self, entry, P, shape, want_db=True, wide=False):
        self.entry, self.P, self.shape, self.want_db = entry, P, shape, want_db
        n_out, n_in = shape
        self.ldw, self.col0 = DW_SHAPES[shape]
        self.half = entry.startswith('h')
        self.layout = int(entry[1]) if self.half else 0
        dZ, X = (T(a) for a in dw_operands(P, n_out, n_in))
        self.amax = None
        if self.half:
            nip = 64 if n_in <= 64 else n_in
            Xp = torch.zeros(P, nip, device=dev())
            Xp[:, :n_in] = X
            X = Xp.half()
            dZ = dZ if n_out <= 4 else (dZ * 8).half()
            self.ldz, self.ldx = n_out, nip
            if self.layout & 1:
                dZ = to_blocked(dZ)                                  # zero padding rows, as the chain writes them
            if self.layout & 2:                                     # padding rows: copies of row P - 1, as the forward writes them
                X = to_blocked(torch.cat([X, X[P - 1:P].expand(pad128(P) - P, nip)]))
            self.dZ, self.X = dZ.reshape(-1), X.reshape(-1)
            self.zshape, self.xshape = tuple(dZ.shape), tuple(X.shape)
            self.scale = None if n_out <= 4 else np.array([4.0], F)
        else:
            self.ldz, self.ldx = (n_out + 8, n_in + 8) if wide else (n_out, n_in)
            self.dZ, self.X = tight(dZ, self.ldz), tight(X, self.ldx)
            if entry == 'f16x3':
                self.amax = np.linspace(0.25, 1.0, AMAX_SLOTS).astype(F) * F(np.abs(dw_operands(P, n_out, n_in)[0]).max())
        self.mask = block_columns(n_out, n_in, self.ldw)

    def need(self, lib):
        fn = lib.hnrf_mlp_dw_h_workspace_bytes if self.half else lib.hnrf_mlp_dw_workspace_bytes
        return fn(self.P, *self.shape)

    def run(self, lib, c, ws=None, ws_bytes=None, misalign=0):
        """-> rc.  ``ws``: a GuardedBuffer to run in instead of a fresh workspace of exactly the stated size."""
        n_out, n_in = self.shape
        need = self.need(lib)
        assert need > 0
        if ws is None:
            ws_bytes = need if ws_bytes is None else ws_bytes
            c.new('ws', ws_bytes, misalign)
        else:
            c.g['ws'], ws_bytes = ws, ws.nbytes
            assert need <= ws_bytes
        dZ, X = c.put('dZ', self.dZ), c.put('X', self.X)
        c.new('dW', 4 * ((n_out - 1) * self.ldw + n_in), misalign=4 * self.col0 % 256)
        dW, db = c.g['dW'].ptr, c.new('db', 4 * n_out) if self.want_db else None
        if self.half:
            return lib.hnrf_mlp_dw_h(dZ, self.ldz, X, self.ldx, self.P, n_out, n_in, self.layout, c.put('scale', self.scale),
                                     dW, self.ldw, db, c.g['ws'].ptr, ws_bytes, _stream())
        return lib.hnrf_mlp_dw(dZ, self.ldz, X, self.ldx, self.P, n_out, n_in, 1 if self.entry == 'f16x3' else 0,
                               c.put('amax', self.amax), 0 if self.amax is None else AMAX_SLOTS, dW, self.ldw, db,
                               c.g['ws'].ptr, ws_bytes, _stream())

    def ops(self):
        """-> (the block's elements in the order of the tight buffer, db or None) through the wrapper, written into a
        block of a NaN-filled (n_out, ldw) matrix."""
        from humannerf_amd import ops
        n_out, n_in = self.shape
        big = torch.full((n_out, self.ldw), float('nan'), device=dev())
        view = big[:, self.col0:self.col0 + n_in]
        if self.half:
            _, db = ops.mlp_dw_h(self.dZ.view(self.zshape), self.X.view(self.xshape), view, self.want_db, T(self.scale), n_in,
                                 self.P, bool(self.layout & 1), bool(self.layout & 2))
        else:
            _, db = ops.mlp_dw(strided(self.dZ, self.P, self.ldz, n_out), strided(self.X, self.P, self.ldx, n_in), view,
                               self.want_db, self.entry, T(self.amax))
        torch.cuda.synchronize()
        out = torch.ones_like(big, dtype=torch.bool)
        out[:, self.col0:self.col0 + n_in] = False
        assert bool(torch.isnan(big[out]).all())                   # the wrapper's call leaves the other columns too
        return view.reshape(-1), db

    def check(self, a, b, want=None):
        """(b), (c) and (d) of two finished cases of this call."""
        n = self.mask.numel()
        names = ['db'] if self.want_db else []
        same(a, b, names)
        same(a, b, ['dW'], rows=self.mask, n_rows=n, row_bytes=4)
        for c in (a, b):
            c.g['dW'].rows_hold_fill(~self.mask, n, 4)
            assert bool(torch.isfinite(c.f('dW')[self.mask]).all())
        if want is not None:
            assert torch.equal(bits(a.f('dW')[self.mask]), bits(want[0]))
            if self.want_db:
                assert torch.equal(bits(a.f('db')), bits(want[1]))


def dw_three_runs(lib, first, second):
    """``first`` under both fills; then ``second`` in the first run's workspace directly after it, equal to ``second``
    in a fresh workspace (no stale slice partial is read); then ``first`` again in that workspace, equal to itself."""
    a, b = both(lambda c: ok(first.run(lib, c), 'first'))
    first.check(a, b, first.ops())
    reuse, fresh, third = (Case(fill, GUARD) for fill in (gb.FILLS[0], gb.FILLS[1], gb.FILLS[1]))
    ok(second.run(lib, reuse, ws=a.g['ws']), 'second call in the same workspace')
    ok(second.run(lib, fresh), 'second call, fresh')
    ok(first.run(lib, third, ws=a.g['ws']), 'first call again')
    reuse.done(), fresh.done(), third.done()
    second.check(reuse, fresh)
    first.check(a, third)


# split-f16 is built for the matrix-shaped layers; the other shapes run the fp32 kernels in either mode
DW_ENTRIES = [(s, e) for s in DW_SHAPES for e in (['f32', 'f16x3'] if matrix_shaped(*s) else ['f32'])]


@pytest.mark.parametrize('P', [P0, 1])
@pytest.mark.parametrize('shape,entry', DW_ENTRIES, ids=['%dx%d-%s' % (s + (e,)) for s, e in DW_ENTRIES])
def test_mlp_dw(shape, entry, P):
    """hnrf_mlp_dw: the dW buffer is TIGHT -- (n_out - 1) * ldw + n_in floats from the block's first element, at the
    block's own alignment -- and the columns of each row outside the block hold the fill; db present and NULL; row
    strides equal to and larger than the widths with tight dZ / X buffers of (P - 1) * ld + width elements; the
    workspace exactly hnrf_mlp_dw_workspace_bytes."""
    lib = lib_train()
    P2, shape2 = other_call(lib.hnrf_mlp_dw_workspace_bytes, P, shape)
    for want_db, wide in itertools.product((True, False), (False, True)):
        first = DwCall(entry, P, shape, want_db, wide)
        if want_db and not wide:
            dw_three_runs(lib, first, DwCall('f32', P2, shape2, True, True))
        else:
            a, b = both(lambda c: ok(first.run(lib, c), 'hnrf_mlp_dw'))
            first.check(a, b, first.ops())


def dwh_layouts(shape):
    n_out, n_in = shape
    if n_out <= 4:
        return ['h0', 'h2']                                        # heads: fp32 dZ; X row-major, X blocked
    return ['h0', 'h1', 'h3'] if n_in > 64 else ['h0', 'h1']      # a blocked X needs n_in 128 | 256


@pytest.mark.parametrize('P', [P0, 1, 129])
@pytest.mark.parametrize('shape', DW_SHAPES, ids=DW_IDS)
def test_mlp_dw_h(shape, P):
    """hnrf_mlp_dw_h in the layouts it is built for -- none, dZ blocked, both blocked; the heads with X row-major and
    blocked --: a blocked matrix is [ceil(P / 128) * 128][W] halves, a row-major one [P][64 | 128 | 256].  P = 129 is one
    row into the second 128-block."""
    lib = lib_train()
    P2, shape2 = other_call(lib.hnrf_mlp_dw_h_workspace_bytes, P, shape)
    for k, entry in enumerate(dwh_layouts(shape)):
        first = DwCall(entry, P, shape, want_db=k != 1)
        if k == 0:
            dw_three_runs(lib, first, DwCall(dwh_layouts(shape2)[-1], P2, shape2))
        else:
            a, b = both(lambda c: ok(first.run(lib, c), 'hnrf_mlp_dw_h'))
            first.check(a, b, first.ops())


@pytest.mark.parametrize('entry', ['f32', 'h1'])
def test_mlp_dw_refuses(entry):
    """A workspace one byte short is HNRF_E_WORKSPACE, one 4 bytes off its 256-byte alignment HNRF_E_ARG; nothing is
    written."""
    lib = lib_train()
    call = DwCall(entry, P0, (256, 256))
    need = call.need(lib)
    for kw, rc in ((dict(ws_bytes=need - 1), E_WORKSPACE), (dict(misalign=4), E_ARG)):
        for fill in gb.FILLS:
            c = Case(fill, GUARD)
            assert call.run(lib, c, **kw) == rc, (kw, lib.hnrf_last_error())
            c.done()
            for k in ('dW', 'db', 'ws'):
                c.g[k].holds_fill()


# ================================================================================================ around the MLPs
def composite_call(lib, c, pr, R, S, with_ad, sized=None):
    """hnrf_composite_bwd on the first R rays of ``pr``; the buffers are sized for ``sized`` rays (default R)."""
    n = R if sized is None else sized
    opt = [c.put('g_a', pr['g_a'][:n]), c.put('g_d', pr['g_d'][:n])] if with_ad else [None, None]
    return lib.hnrf_composite_bwd(c.put('raw', pr['raw'][:n]), c.put('mask', pr['mask'][:n]), c.put('z', pr['z'][:n]),
                                  c.put('rays_d', pr['rays_d'][:n]), c.put('bg', pr['bg']), c.put('g_rgb', pr['g_rgb'][:n]), *opt,
                                  R, S, c.new('d_raw', 16 * n * S), c.new('d_mask', 4 * n * S), _stream())


@pytest.mark.parametrize('with_ad', [True, False], ids=['alpha_depth', 'rgb_only'])
@pytest.mark.parametrize('S', [21, 300])
def test_composite_bwd(S, with_ad):
    """hnrf_composite_bwd at R = 37: S = 21 in one lane group, S = 300 with a ragged last lane; g_alpha / g_depth given
    and NULL.  z_vals[p + 1] of the last sample of the last ray lies behind the input."""
    from humannerf_amd import ops
    lib = lib_train()
    pr = composite_problem(R0, S, 'sparse', seed=5 + S)
    a, b = both(lambda c: ok(composite_call(lib, c, pr, R0, S, with_ad), 'hnrf_composite_bwd'))
    same(a, b, ['d_raw', 'd_mask'])
    opt = (T(pr['g_a']), T(pr['g_d'])) if with_ad else (None, None)
    d_raw, d_mask = ops.composite_bwd(*[T(pr[n]) for n in ('raw', 'mask', 'z', 'rays_d', 'bg', 'g_rgb')], *opt)
    eqb(a, 'd_raw', d_raw), eqb(a, 'd_mask', d_mask)


def test_composite_bwd_writes_nothing_without_rays_or_when_refused():
    """R == 0 writes nothing (outputs of zero bytes, and outputs sized for 37 rays); S = 513 is HNRF_E_UNSUPPORTED and
    writes nothing."""
    lib = lib_train()
    pr = composite_problem(R0, S0, 'sparse')
    both(lambda c: ok(composite_call(lib, c, pr, 0, S0, True), 'hnrf_composite_bwd'))
    for c in both(lambda c: ok(composite_call(lib, c, pr, 0, S0, True, sized=R0), 'hnrf_composite_bwd')):
        c.g['d_raw'].holds_fill(), c.g['d_mask'].holds_fill()
    big = composite_problem(3, 513, 'sparse')
    for fill in gb.FILLS:
        c = Case(fill, GUARD)
        assert composite_call(lib, c, big, 3, 513, True) == E_UNSUPPORTED, lib.hnrf_last_error()
        c.done()
        c.g['d_raw'].holds_fill(), c.g['d_mask'].holds_fill()


PE_ENCODERS = {'fourier10': (10, 1, None), 'hann6': (6, 0, np.array([1, 1, 0.7, 0.2, 0, 0], F))}


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('encoder', PE_ENCODERS)
@pytest.mark.parametrize('P', [P0, 1, 0])
def test_pe_bwd(P, encoder, accumulate):
    """hnrf_pe_bwd for both encoders: 10 bands with the input, 6 bands with the Hann window.  accumulate = 1: dx is an
    input-output, both fills start from the same contents."""
    from humannerf_amd import ops
    lib = lib_train()
    nb, inc, hw = PE_ENCODERS[encoder]
    rs = np.random.RandomState(40 + P)
    x = rs.uniform(-1.2, 1.2, (P, 3)).astype(F)
    g = rs.randn(P, 3 * inc + 6 * nb).astype(F)
    pre = rs.randn(P, 3).astype(F)

    def call(c):
        dx = c.new('dx', 12 * P)
        if accumulate and P:
            c.f('dx', P, 3).copy_(T(pre))
        ok(lib.hnrf_pe_bwd(c.put('x', x) if P else c.new('x', 0), c.put('g', g) if P else c.new('g', 0), c.put('hann', hw), P,
                           nb, inc, accumulate, dx, _stream()), 'hnrf_pe_bwd')
    a, b = both(call)
    same(a, b, ['dx'])
    if P:
        eqb(a, 'dx', ops.pe_bwd(T(x), T(g), T(hw), nb, bool(inc), out=T(pre) if accumulate else None))


def _case_size(case):
    B, G, S, R, extra = case[0]
    return B * S * R


WARP_CASES = ['global-' + min(wrefs.GLOBAL_CASES, key=lambda k: _case_size(wrefs.GLOBAL_CASES[k])),
              'lds-' + min(wrefs.LDS_CASES, key=lambda k: _case_size(wrefs.LDS_CASES[k]))]


@pytest.mark.parametrize('name', WARP_CASES)
def test_sample_warp_bwd(name):
    """hnrf_sample_warp_bwd on the smallest case of each path of tests/test_warp_bwd_refs.py (fewest samples x bones):
    d_vol is [B,G,G,G] -- the bone channels only; the caller owns the background channel's gradient, which the wrapper
    returns as zeros --, vol holds the B bone channels.  The outputs are sums of float atomics: each run is finite and
    within that file's bound of the fp64 reference."""
    from humannerf_amd import ops
    lib = lib_train()
    pr, r64, r32 = wrefs.references(name)
    assert wrefs.takes_lds_path(pr) == name.startswith('lds-')
    B, G, R, S = pr['B'], pr['G'], pr['R'], pr['S']
    keys = ('rays_o', 'rays_d', 'z', 'Rs', 'Ts', 'vol', 'bmin', 'bscale', 'x_skel', 'fg_mask', 'g_x', 'g_mask')

    def call(c):
        ins = [c.put(k, pr[k][:B] if k == 'vol' else pr[k]) for k in keys]
        ok(lib.hnrf_sample_warp_bwd(*ins, R, S, B, G, c.new('d_vol', 4 * B * G ** 3), c.new('d_Rs', 36 * B), c.new('d_Ts', 12 * B),
                                    _stream()), 'hnrf_sample_warp_bwd')
    runs = [dict(vol=c.f('d_vol', B, G, G, G).cpu(), Rs=c.f('d_Rs', B, 3, 3).cpu(), Ts=c.f('d_Ts', B, 3).cpu()) for c in both(call)]
    d_vol, d_Rs, d_Ts = ops.sample_warp_bwd(*(T(pr[k]) for k in keys))
    torch.cuda.synchronize()
    assert d_vol.shape[0] == B + pr['extra'] and bool((d_vol[B:] == 0).all())    # the channels beyond the bones: zeros
    runs.append(dict(vol=d_vol[:B].cpu(), Rs=d_Rs.cpu(), Ts=d_Ts.cpu()))
    for got in runs:
        for k, (err, tol, floor) in wrefs.errors(got, r64, r32).items():
            assert bool(torch.isfinite(got[k]).all()), (name, k)
            assert err <= tol, (name, k, err, tol, floor)


# ------------------------------------------------------------------------------------------------ kinematics
def basis_problem(seed=0):
    from humannerf_amd import scene
    rs = np.random.RandomState(seed)
    dst_Rs, dst_Ts = scene.body_pose_to_body_RTs(rs.randn(72) * 0.4, scene.TPOSE_JOINTS)
    gt = scene.get_canonical_global_tfms(scene.TPOSE_JOINTS)
    return dict(dst_Rs=dst_Rs.astype(F), dst_Ts=dst_Ts.astype(F), gt=gt.astype(F), rvec=(rs.randn(23, 3) * 0.3).astype(F),
                g_Rs=rs.randn(24, 3, 3).astype(F), g_Ts=rs.randn(24, 3).astype(F))


def basis_fwd(lib, c, pr, refined, saved=True, B=24, misalign=0):
    ins = [c.put(k, pr[k]) for k in ('dst_Rs', 'dst_Ts', 'gt')]
    sv = c.new('saved', lib.hnrf_motion_basis_saved_bytes(), misalign) if saved else None
    outs = [c.new('Rs', 36 * 24), c.new('Ts', 12 * 24), sv]
    if refined:
        return lib.hnrf_refined_motion_basis_fwd(c.put('rvec', pr['rvec']), *ins, B, *outs, _stream())
    return lib.hnrf_motion_basis_fwd(*ins, B, *outs, _stream())


def basis_bwd(lib, c, pr, refined, B=24, misalign=0):
    """The backward after the forward that fills ``saved`` in the same case (B and the alignment: of the backward)."""
    fresh = Case(c.fill, GUARD)
    if misalign:                                                   # the forward refuses such a buffer: copy a good one's bytes
        ok(basis_fwd(lib, fresh, pr, refined), 'forward')
        c.new('saved', lib.hnrf_motion_basis_saved_bytes(), misalign)
        c.g['saved'].interior_bytes().copy_(fresh.done().g['saved'].interior_bytes())
    else:
        ok(basis_fwd(lib, c, pr, refined), 'forward')
        del c.g['Rs'], c.g['Ts']
    c.orig['saved'] = c.g['saved'].interior_bytes().clone()        # an input of the backward
    g = [c.put(k, pr[k]) for k in ('g_Rs', 'g_Ts')]
    ins = [c.g[k].ptr for k in ('dst_Rs', 'dst_Ts', 'gt')] if not misalign else [c.put(k, pr[k]) for k in ('dst_Rs', 'dst_Ts', 'gt')]
    outs = [c.new('d_Rs', 36 * 24), c.new('d_Ts', 12 * 24)]
    if refined:
        rv = c.g['rvec'].ptr if not misalign else c.put('rvec', pr['rvec'])
        return lib.hnrf_refined_motion_basis_bwd(*g, rv, *ins, B, c.g['saved'].ptr, c.new('d_rvec', 12 * 23), *outs, _stream())
    return lib.hnrf_motion_basis_bwd(*g, *ins, B, c.g['saved'].ptr, *outs, _stream())


@pytest.mark.parametrize('refined', [False, True], ids=['plain', 'refined'])
def test_motion_basis(refined):
    """hnrf_motion_basis_fwd / _bwd and the refined pair: saved is exactly hnrf_motion_basis_saved_bytes() (on the
    forward also NULL); the backward's outputs do not depend on what saved held before the forward."""
    from humannerf_amd import ops
    lib = lib_train()
    assert lib.hnrf_motion_basis_saved_bytes() == 2 * 24 * 16 * 8
    pr = basis_problem()
    t = {k: T(v) for k, v in pr.items()}
    rv = t['rvec'] if refined else None
    Rs, Ts, saved = ops.motion_basis_fwd(t['dst_Rs'], t['dst_Ts'], t['gt'], want_saved=True, rvec=rv)
    for with_saved in (True, False):
        a, b = both(lambda c: ok(basis_fwd(lib, c, pr, refined, with_saved), 'forward'))
        same(a, b, ['Rs', 'Ts'])
        eqb(a, 'Rs', Rs), eqb(a, 'Ts', Ts)
    want = ops.motion_basis_bwd(t['g_Rs'], t['g_Ts'], t['dst_Rs'], t['dst_Ts'], t['gt'], saved, rvec=rv)
    names = ['d_Rs', 'd_Ts'] + (['d_rvec'] if refined else [])
    a, b = both(lambda c: ok(basis_bwd(lib, c, pr, refined), 'backward'))
    same(a, b, names)
    for n, w in zip(names, want):
        eqb(a, n, w)


@pytest.mark.parametrize('refined', [False, True], ids=['plain', 'refined'])
def test_motion_basis_refuses(refined):
    """A saved that is 4-byte but not 8-byte aligned is HNRF_E_ARG, B = 23 HNRF_E_UNSUPPORTED, forward and backward;
    nothing is written."""
    lib = lib_train()
    pr = basis_problem()
    for kw, rc in ((dict(misalign=4), E_ARG), (dict(B=23), E_UNSUPPORTED)):
        for fill in gb.FILLS:
            c = Case(fill, GUARD)
            assert basis_fwd(lib, c, pr, refined, **kw) == rc, (kw, lib.hnrf_last_error())
            c.done()
            for k in ('Rs', 'Ts', 'saved'):
                c.g[k].holds_fill()
            c = Case(fill, GUARD)
            assert basis_bwd(lib, c, pr, refined, **kw) == rc, (kw, lib.hnrf_last_error())
            c.done()
            for k in ['d_Rs', 'd_Ts'] + (['d_rvec'] if refined else []):
                c.g[k].holds_fill()


POSE_DIMS = [[69, 256, 256, 256, 256, 69], [5, 7, 3], [12, 9]]


def pose_problem(dims):
    rs = np.random.RandomState(len(dims) + dims[0])
    L = len(dims) - 1
    return dict(Ws=[(rs.randn(dims[l + 1], dims[l]) / np.sqrt(dims[l])).astype(F) for l in range(L)],
                bs=[(rs.randn(dims[l + 1]) * 0.1).astype(F) for l in range(L)], x=rs.randn(dims[0]).astype(F),
                g=rs.randn(dims[-1]).astype(F))


def pose_fwd(lib, c, pr, dims, saved=True):
    L = len(dims) - 1
    W = (ctypes.c_void_p * L)(*[c.put('W%d' % l, w) for l, w in enumerate(pr['Ws'])])
    b = (ctypes.c_void_p * L)(*[c.put('b%d' % l, v) for l, v in enumerate(pr['bs'])])
    sv = c.new('saved', lib.hnrf_pose_mlp_saved_bytes(L)) if saved else None
    rc = lib.hnrf_pose_mlp_fwd(c.put('x', pr['x']), W, b, (ctypes.c_int * len(dims))(*dims), L, c.new('out', 4 * dims[-1]), sv,
                               _stream())
    return rc, W, b


@pytest.mark.parametrize('dims', POSE_DIMS, ids=['default', '5-7-3', '12-9'])
def test_pose_mlp(dims):
    """hnrf_pose_mlp_fwd / _bwd: every W[l], b[l], dW[l] and db[l] in a buffer of its own, saved exactly
    hnrf_pose_mlp_saved_bytes(layers) (one layer: NULL on the forward), d_x_parts [8][256] given and NULL.  Its first
    ceil(dims[1] / 32) rows, columns < dims[0], are written; everything else in it holds the fill.  The backward does not
    depend on the unwritten tail of each 256-float slot of saved."""
    from humannerf_amd import ops
    lib = lib_train()
    L = len(dims) - 1
    pr = pose_problem(dims)
    assert lib.hnrf_pose_mlp_saved_bytes(L) == (L - 1 + 16) * 256 * 4
    Ws, bs = [T(w) for w in pr['Ws']], [T(b) for b in pr['bs']]
    out, saved = ops.pose_mlp_fwd(T(pr['x']), Ws, bs)
    for with_saved in ([True, False] if L == 1 else [True]):
        a, b = both(lambda c: ok(pose_fwd(lib, c, pr, dims, with_saved)[0], 'hnrf_pose_mlp_fwd'))
        same(a, b, ['out'])
        eqb(a, 'out', out)
    dW, db, d_x = ops.pose_mlp_bwd(T(pr['g']), T(pr['x']), Ws, bs, saved, want_dx=True)
    torch.cuda.synchronize()
    n_parts = (dims[1] + 31) // 32
    written = torch.zeros(8, 256, dtype=torch.bool, device=dev())
    written[:n_parts, :dims[0]] = True
    for with_parts in (True, False):
        def call(c):
            rc, W, b = pose_fwd(lib, c, pr, dims)
            ok(rc, 'hnrf_pose_mlp_fwd')
            del c.g['out']
            gW = (ctypes.c_void_p * L)(*[c.new('dW%d' % l, 4 * dims[l + 1] * dims[l]) for l in range(L)])
            gb_ = (ctypes.c_void_p * L)(*[c.new('db%d' % l, 4 * dims[l + 1]) for l in range(L)])
            ok(lib.hnrf_pose_mlp_bwd(c.put('g', pr['g']), c.g['x'].ptr, W, b, (ctypes.c_int * len(dims))(*dims), L, c.g['saved'].ptr,
                                     gW, gb_, c.new('parts', 4 * 8 * 256) if with_parts else None, _stream()), 'hnrf_pose_mlp_bwd')
        a, b = both(call)
        names = ['dW%d' % l for l in range(L)] + ['db%d' % l for l in range(L)]
        same(a, b, names)
        for l in range(L):
            eqb(a, 'dW%d' % l, dW[l]), eqb(a, 'db%d' % l, db[l])
        if with_parts:
            same(a, b, ['parts'], rows=written.reshape(-1), n_rows=8 * 256, row_bytes=4)
            for c in (a, b):
                c.g['parts'].rows_hold_fill(~written.reshape(-1), 8 * 256, 4)
            assert torch.equal(bits(a.f('parts', 8, 256)[:n_parts, :dims[0]].sum(0)), bits(d_x))


# ------------------------------------------------------------------------------------------------ the volume decoder's fold
@pytest.mark.parametrize('cout,dims,biases', [(5, (3, 2, 4), (True, False)), (25, (16, 16, 16), (True,))], ids=['ragged', 'last_layer'])
def test_deconv_fold(cout, dims, biases):
    """hnrf_deconv_fold: col [D H W, cout 64], bias [cout] or NULL -> out [cout, 2D, 2H, 2W]; the ragged case of
    tests/test_gpu_grad.py::test_decoder_layers_as_gemm_plus_fold_kernel and the decoder's 25-channel layer on 16^3."""
    from humannerf_amd import ops
    lib = lib_train()
    D, H, W = dims
    rs = np.random.RandomState(cout)
    col, bias = rs.randn(D * H * W, cout * 64).astype(F), rs.randn(cout).astype(F)
    for with_bias in biases:
        a, b = both(lambda c: ok(lib.hnrf_deconv_fold(c.put('col', col), c.put('bias', bias) if with_bias else None, cout, D, H, W,
                                                      c.new('out', 4 * cout * 8 * D * H * W), _stream()), 'hnrf_deconv_fold'))
        same(a, b, ['out'])
        eqb(a, 'out', ops.deconv_fold(T(col), T(bias) if with_bias else None, cout, D, H, W))
