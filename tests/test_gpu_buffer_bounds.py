"""Where the inference kernels write and read: every input and output of every call sits in a guarded buffer
(tests/guarded_buffers.py) of EXACTLY the size include/hnrf.h states, the call runs once under each of the two fills,
and

  (a) every guard is intact,
  (b) every output is bit-equal between the two fills (an element never written, a result computed from what a buffer
      held before the call or from bytes behind an input's end differs),
  (c) every output is bit-equal to the same operation through the ops wrapper on allocator-provided buffers,
  (d) the rows the header calls "not written" / "untouched" still hold the fill, and an entry that returns without a
      launch or refuses its arguments leaves everything at the fill,
  (e) every input holds what it held; a packed image may only gain HNRF_STATUS_F16_RANGE in its status word.

There is no tolerance in this file: every comparison is on bit patterns.  The values themselves are checked elsewhere
(tests/test_gpu_render_kernels.py and the files beside it).  Shapes: R = 37 rays of S = 21 samples, P = 777 -- no
multiple of 32, 64, 128 or 256, so 3P, 4P and P B floats all end off a 16-byte and a 256-byte boundary.  The C entries
are called through humannerf_amd._lib with raw pointers.  Needs an MI355X: ``pytest -m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

from humannerf_amd import shared_input as si
from tests import guarded_buffers as gb
from tests.guarded_case import Case, T, _stream, bits, both, dev, eq, ok, same
from tests import multihead_cases as mc
from tests import test_render_kernel_refs as refs
from tests.test_train_kernel_refs import CNL_NAMES, NR_NAMES

pytestmark = pytest.mark.gpu

F = np.float32
R0, S0 = 37, 21
P0 = R0 * S0
E_ARG, E_WORKSPACE = -1, -4
MODES = ['f32', 'f16x3']
BMW = 'backward_motion_weights'
# a representative of the seeded network's size for the share kernels (tests/test_gpu_shared_input.py); c_xyz = +0 + c_off
C_OFF = np.array([-0.0686608, -0.00916304, 0.06966332], F)
C_XYZ = (np.zeros(3, F) + C_OFF).astype(F)


def lib_all():
    """The library with the entries of every header this file calls bound."""
    from humannerf_amd import _lib
    _lib.load_heads()
    return _lib.load_heads_shared()


def off_threshold(m, eps):
    """``m`` with every value within 1e-3 of the threshold ``eps`` moved 1e-2 above it: the test makes its masks, and no
    sample may sit where a rounding decides its class."""
    near = np.abs(m - eps) < 1e-3
    return np.where(near, m + F(1e-2), m).astype(F)


# ------------------------------------------------------------------------------------------------ the weights
@pytest.fixture(scope='module')
def state(seeded_params):
    from humannerf_amd.seeded import with_density
    return with_density(seeded_params, bias_delta=-10.0)


def _image(lib, t, which, mode):
    from humannerf_amd import ops
    m = ops.MLP_MODES[mode]
    nbytes = (lib.hnrf_canonical_packed_bytes if which == 'canonical' else lib.hnrf_nonrigid_packed_bytes)(m)
    off = (lib.hnrf_canonical_status_offset if which == 'canonical' else lib.hnrf_nonrigid_status_offset)(m)
    assert 0 < nbytes <= t.numel() * 4 and off + 4 <= nbytes and off % 4 == 0
    return t, nbytes, off


@pytest.fixture(scope='module')
def mlps(state):
    """Per mode: the packed images (tensor, exact bytes, status offset) of the seeded state -- 'nr', 'cnl', ('heads', H) --
    and the Hann weights and the frame's condition code."""
    from humannerf_amd import _lib, ops
    lib = _lib.load_heads()
    cond = T((np.random.RandomState(3).randn(69) * 0.2).astype(F))
    out = {'hann': np.ones(6, F)}
    for mode in MODES:
        nw, nb = [T(state[n + '.weight']) for n in NR_NAMES], [T(state[n + '.bias']) for n in NR_NAMES]
        cw, cb = [T(state[n + '.weight']) for n in CNL_NAMES], [T(state[n + '.bias']) for n in CNL_NAMES]
        out[mode] = {'nr': _image(lib, ops.nonrigid_pack(nw, nb, cond, mode), 'nonrigid', mode),
                     'cnl': _image(lib, ops.canonical_pack(cw, cb, mode), 'canonical', mode)}
        for H in (2, 3, 8):
            hs = mc.multihead_state(state, H)
            hw, hb = [T(hs[n + '.weight']) for n in CNL_NAMES], [T(hs[n + '.bias']) for n in CNL_NAMES]
            out[mode]['heads', H] = _image(lib, ops.canonical_heads_pack(hw, hb, H, mode), 'canonical', mode)
    torch.cuda.synchronize()
    return out


def positions(P, seed=0):
    """[P,3] host-made sample positions inside and around the unit box."""
    return (np.random.RandomState(100 + seed).randn(P, 3) * 0.6).astype(F)


def listed(P, n, seed=0):
    """(idx [P] int32 with -1 behind the n listed samples -- entries the kernels must not read --, count [1], the boolean
    mask of the listed rows)."""
    perm = np.random.RandomState(7 * P + n + seed).permutation(P)[:n]
    idx = np.full(P, -1, np.int32)
    idx[:n] = perm
    m = np.zeros(P, bool)
    m[perm] = True
    return idx, np.array([n], np.int32), torch.from_numpy(m).to(dev())


# a list that ends inside a tile of every kernel (32 NW, 128, 256) after at least one full one: 0 < 333 < 777
MANY = 333
SPARSE_COUNTS = [0, 1, 128, 129, MANY]


def check_counts(P, n):
    assert 0 <= n <= P
    if n == MANY:
        assert 0 < n < P and n >= 256 and all(n % t for t in (32, 64, 128, 256))


# ================================================================================================ 2. per-kernel contracts
# ------------------------------------------------------------------------------------------------ K1
def k1_inputs(c, pr, use_t):
    """The ten leading pointers of K1 and of every render entry.  vol holds the B bone channels only: the header says
    the background channel is not read."""
    B = pr['B']
    return ([c.put(k, pr[k].reshape(-1) if k in ('near', 'far') else pr[k]) for k in ('rays_o', 'rays_d', 'near', 'far')]
            + [c.put('t_rand', pr['t_rand']) if use_t else None]
            + [c.put(k, pr[k][:B] if k == 'vol' else pr[k]) for k in ('Rs', 'Ts', 'vol', 'bmin', 'bscale')])


def k1_outputs(c, P, B, want_bmw):
    return [c.new('z', 4 * P), c.new('x_skel', 12 * P), c.new('mask', 4 * P), c.new('bmw', 4 * P * B) if want_bmw else None]


def ops_k1(pr, use_t, want_bmw):
    from humannerf_amd import ops
    B = pr['B']
    out = ops.sample_warp(T(pr['rays_o']), T(pr['rays_d']), T(pr['near']), T(pr['far']), T(pr['t_rand']) if use_t else None,
                          T(pr['Rs']), T(pr['Ts']), T(pr['vol'][:B]), T(pr['bmin']), T(pr['bscale']), pr['S'], want_bmw=want_bmw)
    torch.cuda.synchronize()
    return dict(zip(('z', 'x_skel', 'mask', 'bmw'), out))


@pytest.mark.parametrize('want_bmw', [False, True], ids=['nobmw', 'bmw'])
@pytest.mark.parametrize('use_t', [False, True], ids=['linspace', 't_rand'])
@pytest.mark.parametrize('B,G', [(24, 16), (7, 33)], ids=['B24', 'B7'])
def test_sample_warp(B, G, use_t, want_bmw):
    """hnrf_sample_warp_fwd: the 16-byte stores of bmw (B = 24) and the 4-byte ones (B = 7, odd lattice), t_rand null and
    given, bmw null and given."""
    from humannerf_amd import _lib
    lib = _lib.load()
    pr = refs.k1_problem(B, G, S0, R0)
    names = ['z', 'x_skel', 'mask'] + (['bmw'] if want_bmw else [])

    def call(c):
        a = k1_inputs(c, pr, use_t)
        ok(lib.hnrf_sample_warp_fwd(*a, R0, S0, B, G, *k1_outputs(c, P0, B, want_bmw), _stream()), 'hnrf_sample_warp_fwd')
    a, b = both(call)
    same(a, b, names)
    want = ops_k1(pr, use_t, want_bmw)
    for n in names:
        eq(a, n, want[n])


@pytest.mark.parametrize('B,G', [(24, 16), (7, 33)], ids=['B24', 'B7'])
def test_sample_warp_without_rays_and_with_one(B, G):
    """R == 0 returns HNRF_OK without a launch and leaves every output untouched; R = 1, S = 2 is the smallest launch."""
    from humannerf_amd import _lib
    lib = _lib.load()
    pr = refs.k1_problem(B, G, 2, 1)

    def call0(c):
        a = k1_inputs(c, pr, True)
        ok(lib.hnrf_sample_warp_fwd(*a, 0, 2, B, G, *k1_outputs(c, 2, B, True), _stream()), 'hnrf_sample_warp_fwd')
    for c in both(call0):
        for n in ('z', 'x_skel', 'mask', 'bmw'):
            c.g[n].holds_fill()

    def call1(c):
        a = k1_inputs(c, pr, True)
        ok(lib.hnrf_sample_warp_fwd(*a, 1, 2, B, G, *k1_outputs(c, 2, B, True), _stream()), 'hnrf_sample_warp_fwd')
    a, b = both(call1)
    same(a, b, ('z', 'x_skel', 'mask', 'bmw'))
    want = ops_k1(pr, True, True)
    for n in ('z', 'x_skel', 'mask', 'bmw'):
        eq(a, n, want[n])


# ------------------------------------------------------------------------------------------------ compaction
def host_mask(P, seed=0):
    """A host-made fg_mask: values over (0, 1.1), every seventh exactly 0, three NaNs."""
    m = np.random.RandomState(50 + P + seed).uniform(0, 1.1, P).astype(F)
    m[::7] = 0
    if P >= 8:
        m[[1, P // 2, P - 1]] = np.nan
    return m


@pytest.mark.parametrize('eps', [0.0, 0.3])
@pytest.mark.parametrize('P', [0, 1, P0])
def test_compact_samples(P, eps):
    """hnrf_compact_samples: idx[*count .. P) keeps the fill, a NaN is never kept (also at eps == 0), P == 0 sets *count = 0
    and writes nothing else.  The order of the list is the blocks' (an atomic): the SET is compared."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    m = off_threshold(host_mask(P), eps) if P > 1 else np.full(P, 0.5, F)
    keep = ~np.isnan(m) & (m >= eps)
    n = int(keep.sum())
    if P == P0:
        assert 0 < n < P and n >= 256 and n % 256 and np.isnan(m).any() and (np.abs(m[~np.isnan(m)] - eps) > 1e-4).all()

    def call(c):
        ok(lib.hnrf_compact_samples(c.put('mask', m) if P else c.new('mask', 0), eps, P, c.new('idx', 4 * P),
                                    c.new('count', 4), _stream()), 'hnrf_compact_samples')
    a, b = both(call)
    for c in (a, b):
        assert int(c.i('count')[0]) == n
        assert np.array_equal(np.sort(c.i('idx').cpu().numpy()[:n]), np.nonzero(keep)[0])
        if P:
            c.g['idx'].rows_hold_fill(torch.arange(n, P), P, 4)
    if P:
        idx, count = ops.compact_samples(T(m), eps)
        assert int(count.item()) == n and np.array_equal(np.sort(idx.cpu().numpy()[:n]), np.nonzero(keep)[0])


def share_x(P):
    """Host-made x_skel with both classes: 40 % of the rows underflow (+-0, +-1e-45, +-2^-40: shared under C_OFF), the
    others are of the size of a body (live)."""
    rs = np.random.RandomState(P)
    x = (rs.randn(P, 3) * 0.4 + 0.01).astype(F)
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 2.0 ** -40, -2.0 ** -40], F)
    rows = rs.uniform(0, 1, P) < 0.4
    x[rows] = tiny[rs.randint(0, tiny.size, (int(rows.sum()), 3))]
    return x


def check_share(c, P, live, H, lean, c_raw):
    """(d) of the share kernels: the rows of live samples keep the fill in raw (every plane), xyz and offsets; the shared
    rows hold the representative; idx[*count .. P) keeps the fill."""
    n = int(live.sum())
    lv = torch.from_numpy(live).to(dev())
    assert int(c.i('count')[0]) == n
    assert np.array_equal(np.sort(c.i('idx').cpu().numpy()[:n]), np.nonzero(live)[0])
    c.g['idx'].rows_hold_fill(torch.arange(n, P), P, 4)
    for g in range(H):
        c.g['raw'].rows_hold_fill(lv, P, 16, offset=g * P * 16)
        got = c.f('raw', H, P, 4)[g][~lv]
        assert torch.equal(bits(got), bits(T(c_raw.reshape(H, 4)[g])[None].expand(P - n, 4)))
    for k, want in (('offsets', C_OFF), ('xyz', C_XYZ)):
        if not lean:
            c.g[k].rows_hold_fill(lv, P, 12)
            assert torch.equal(bits(c.f(k, P, 3)[~lv]), bits(T(want)[None].expand(P - n, 3)))


@pytest.mark.parametrize('lean', [False, True], ids=['diag', 'lean'])
@pytest.mark.parametrize('P', [0, 1, P0])
def test_share_compact(P, lean):
    """hnrf_share_compact on a host-made x_skel: the rows of live samples are not touched, idx[*count .. P) keeps the
    fill, offsets and xyz both NULL are not written; P == 0 sets *count = 0 without a launch."""
    from humannerf_amd import _lib
    lib = _lib.load()
    x = share_x(P) if P > 1 else np.full((P, 3), 0.25, F)
    c_raw = np.array([0.25, -1.5, 3.0, -0.0], F)
    live = ~si.shared_mask(x, C_OFF, C_XYZ) if P else np.zeros(0, bool)
    if P == P0:
        n = int(live.sum())
        assert 0 < n < P and n >= 256 and n % 256 and n % 32

    def call(c):
        ok(lib.hnrf_share_compact(c.put('x', x) if P else c.new('x', 0), c.put('c_off', C_OFF), c.put('c_xyz', C_XYZ),
                                  c.put('c_raw', c_raw), P, c.new('idx', 4 * P), c.new('count', 4),
                                  None if lean else c.new('offsets', 12 * P), None if lean else c.new('xyz', 12 * P),
                                  c.new('raw', 16 * P), _stream()), 'hnrf_share_compact')
    for c in both(call):
        check_share(c, P, live, 1, lean, c_raw)


@pytest.mark.parametrize('lean', [False, True], ids=['diag', 'lean'])
@pytest.mark.parametrize('want_bmw', [False, True], ids=['nobmw', 'bmw'])
def test_sample_warp_share(want_bmw, lean):
    """hnrf_sample_warp_share_fwd: z_vals / x_skel / fg_mask / bmw as hnrf_sample_warp_fwd writes them, the rows of live
    samples of raw / xyz / offsets keep the fill, idx[*count .. P) keeps the fill.  The classes come from the fp64 K1
    reference: a sample without any weight has x_skel = 0 and is shared, one of the size of a body is live."""
    from humannerf_amd import _lib
    lib = _lib.load()
    B, G = 24, 16
    pr = refs.k1_problem(B, G, S0, R0)
    r = refs.ref_k1(pr, True)
    zero = (r['wsum'] == 0).numpy()
    big = (r['x'].abs().amax(1) > 1e-3).numpy()
    assert (zero | big).all() and not (zero & big).any()               # no sample near the predicate's threshold
    n = int(big.sum())
    assert 0 < n < P0 and n >= 256 and n % 256 and n % 32
    c_raw = np.array([0.25, -1.5, 3.0, -0.0], F)
    names = ['z', 'x_skel', 'mask'] + (['bmw'] if want_bmw else [])

    def call(c):
        a = k1_inputs(c, pr, True)
        ok(lib.hnrf_sample_warp_share_fwd(*a, R0, S0, B, G, *k1_outputs(c, P0, B, want_bmw), c.put('c_off', C_OFF),
                                          c.put('c_xyz', C_XYZ), c.put('c_raw', c_raw), c.new('idx', 4 * P0),
                                          c.new('count', 4), None if lean else c.new('offsets', 12 * P0),
                                          None if lean else c.new('xyz', 12 * P0), c.new('raw', 16 * P0), _stream()),
           'hnrf_sample_warp_share_fwd')
    a, b = both(call)
    same(a, b, names)
    want = ops_k1(pr, True, want_bmw)
    for k in names:
        eq(a, k, want[k])
    for c in (a, b):
        check_share(c, P0, big, 1, lean, c_raw)


@pytest.mark.parametrize('H', [2, 3, 8])
def test_share_heads(H):
    """hnrf_share_compact_heads and hnrf_sample_warp_share_heads_fwd: no plane row of a live sample is touched, the
    shared rows of plane g hold c_raw[g]."""
    lib = lib_all()
    x = share_x(P0)
    live = ~si.shared_mask(x, C_OFF, C_XYZ)
    c_raw = np.random.RandomState(H).randn(H, 4).astype(F)

    def call(c):
        ok(lib.hnrf_share_compact_heads(c.put('x', x), c.put('c_off', C_OFF), c.put('c_xyz', C_XYZ), c.put('c_raw', c_raw),
                                        P0, H, c.new('idx', 4 * P0), c.new('count', 4), c.new('offsets', 12 * P0),
                                        c.new('xyz', 12 * P0), c.new('raw', 16 * P0 * H), _stream()),
           'hnrf_share_compact_heads')
    for c in both(call):
        check_share(c, P0, live, H, False, c_raw)
    for P in (0, 1):                                              # P == 0 sets *count = 0 without a launch
        xs = np.full((P, 3), 0.25, F)

        def small(c):
            ok(lib.hnrf_share_compact_heads(c.put('x', xs) if P else c.new('x', 0), c.put('c_off', C_OFF), c.put('c_xyz', C_XYZ),
                                            c.put('c_raw', c_raw), P, H, c.new('idx', 4 * P), c.new('count', 4),
                                            c.new('offsets', 12 * P), c.new('xyz', 12 * P), c.new('raw', 16 * P * H), _stream()),
               'hnrf_share_compact_heads')
        for c in both(small):
            check_share(c, P, np.ones(P, bool), H, False, c_raw)
    B, G = 24, 16
    pr = refs.k1_problem(B, G, S0, R0)
    big = (refs.ref_k1(pr, False)['x'].abs().amax(1) > 1e-3).numpy()

    def fused(c):
        a = k1_inputs(c, pr, False)
        ok(lib.hnrf_sample_warp_share_heads_fwd(*a, R0, S0, B, G, *k1_outputs(c, P0, B, True), c.put('c_off', C_OFF),
                                                c.put('c_xyz', C_XYZ), c.put('c_raw', c_raw), H, c.new('idx', 4 * P0),
                                                c.new('count', 4), c.new('offsets', 12 * P0), c.new('xyz', 12 * P0),
                                                c.new('raw', 16 * P0 * H), _stream()), 'hnrf_sample_warp_share_heads_fwd')
    a, b = both(fused)
    same(a, b, ('z', 'x_skel', 'mask', 'bmw'))
    want = ops_k1(pr, False, True)
    for k in ('z', 'x_skel', 'mask', 'bmw'):
        eq(a, k, want[k])
    for c in (a, b):
        check_share(c, P0, big, H, False, c_raw)


# ------------------------------------------------------------------------------------------------ K2, K3
@pytest.mark.parametrize('want_offsets', [False, True], ids=['nooffsets', 'offsets'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('P', [1, P0])
def test_nonrigid_dense(mlps, P, mode, want_offsets):
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    x = positions(P)

    def call(c):
        ok(lib.hnrf_nonrigid_fwd(c.put('x', x), c.put('hann', mlps['hann']), c.packed('nr', mlps[mode]['nr']),
                                 ops._mode_arg(mode), P, c.new('xyz', 12 * P), c.new('offsets', 12 * P) if want_offsets else None,
                                 _stream()), 'hnrf_nonrigid_fwd')
    a, b = both(call)
    names = ['xyz'] + (['offsets'] if want_offsets else [])
    same(a, b, names)
    xyz, off = ops.nonrigid(T(x), T(mlps['hann']), mlps[mode]['nr'][0].clone(), mode, want_offsets=want_offsets)
    eq(a, 'xyz', xyz)
    if want_offsets:
        eq(a, 'offsets', off)


@pytest.mark.parametrize('want_offsets', [False, True], ids=['nooffsets', 'offsets'])
@pytest.mark.parametrize('mode', MODES)
def test_nonrigid_sparse(mlps, mode, want_offsets):
    """hnrf_nonrigid_fwd_sparse with *count at 0, 1, 128, 129 (the workgroup return) and 333: the listed rows equal the
    dense launch's; *count == 0 writes nothing.  (That unlisted rows keep what they held is
    tests/test_gpu_render_kernels.py::test_sparse_mlp_launches_equal_dense_on_the_listed_samples.)"""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    P, x = P0, positions(P0)
    xyz, off = ops.nonrigid(T(x), T(mlps['hann']), mlps[mode]['nr'][0].clone(), mode, want_offsets=True)
    names = ['xyz'] + (['offsets'] if want_offsets else [])
    for n in SPARSE_COUNTS:
        check_counts(P, n)
        idx, count, m = listed(P, n)

        def call(c):
            ok(lib.hnrf_nonrigid_fwd_sparse(c.put('x', x), c.put('hann', mlps['hann']), c.packed('nr', mlps[mode]['nr']),
                                            ops._mode_arg(mode), P, c.put('idx', idx), c.put('count', count),
                                            c.new('xyz', 12 * P), c.new('offsets', 12 * P) if want_offsets else None,
                                            _stream()), 'hnrf_nonrigid_fwd_sparse')
        a, b = both(call)
        same(a, b, names, rows=m, n_rows=P, row_bytes=12)
        assert torch.equal(bits(a.f('xyz', P, 3)[m]), bits(xyz[m])), n
        if want_offsets:
            assert torch.equal(bits(a.f('offsets', P, 3)[m]), bits(off[m])), n
        if n == 0:
            for c in (a, b):
                for k in names:
                    c.g[k].holds_fill()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('P', [1, P0])
def test_canonical_dense(mlps, P, mode):
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    x = positions(P, 1)

    def call(c):
        ok(lib.hnrf_canonical_fwd(c.put('xyz', x), c.packed('cnl', mlps[mode]['cnl']), ops._mode_arg(mode), P,
                                  c.new('raw', 16 * P), _stream()), 'hnrf_canonical_fwd')
    a, b = both(call)
    same(a, b, ['raw'])
    eq(a, 'raw', ops.canonical(T(x), mlps[mode]['cnl'][0].clone(), mode))


@pytest.mark.parametrize('mode', MODES)
def test_canonical_sparse(mlps, mode):
    """hnrf_canonical_fwd_sparse, counts as test_nonrigid_sparse."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    P, x = P0, positions(P0, 1)
    raw = ops.canonical(T(x), mlps[mode]['cnl'][0].clone(), mode)
    for n in SPARSE_COUNTS:
        check_counts(P, n)
        idx, count, m = listed(P, n)

        def call(c):
            ok(lib.hnrf_canonical_fwd_sparse(c.put('xyz', x), c.packed('cnl', mlps[mode]['cnl']), ops._mode_arg(mode), P,
                                             c.put('idx', idx), c.put('count', count), c.new('raw', 16 * P), _stream()),
               'hnrf_canonical_fwd_sparse')
        a, b = both(call)
        same(a, b, ['raw'], rows=m, n_rows=P, row_bytes=16)
        assert torch.equal(bits(a.f('raw', P, 4)[m]), bits(raw[m])), n
        if n == 0:
            a.g['raw'].holds_fill(), b.g['raw'].holds_fill()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('H', [2, 3, 8])
def test_canonical_heads(mlps, H, mode):
    """hnrf_canonical_heads_fwd and its sparse form: raw [H][P][4] ends where plane H - 1 ends (H = 3: the `g < n_heads`
    branch with an odd head count), `raw[g * plane + sample]` stays inside its plane; counts as test_nonrigid_sparse.
    (Unlisted rows of every plane: tests/test_gpu_multihead.py::test_heads_sparse_launch.)"""
    from humannerf_amd import _lib, ops
    lib = _lib.load_heads()
    P, x = P0, positions(P0, 2)
    image = mlps[mode]['heads', H]

    def dense(c):
        ok(lib.hnrf_canonical_heads_fwd(c.put('xyz', x), c.packed('cnl', image), ops._mode_arg(mode), P, H,
                                        c.new('raw', 16 * P * H), _stream()), 'hnrf_canonical_heads_fwd')
    a, b = both(dense)
    same(a, b, ['raw'])
    raw = ops.canonical_heads(T(x), image[0].clone(), H, mode)
    eq(a, 'raw', raw)
    for n in SPARSE_COUNTS:
        check_counts(P, n)
        idx, count, m = listed(P, n)

        def sparse(c):
            ok(lib.hnrf_canonical_heads_fwd_sparse(c.put('xyz', x), c.packed('cnl', image), ops._mode_arg(mode), P, H,
                                                   c.put('idx', idx), c.put('count', count), c.new('raw', 16 * P * H),
                                                   _stream()), 'hnrf_canonical_heads_fwd_sparse')
        a, b = both(sparse)
        for g in range(H):
            same(a, b, ['raw'], rows=m, n_rows=P, row_bytes=16, offset=g * P * 16)
        assert torch.equal(bits(a.f('raw', H, P, 4)[:, m]), bits(raw[:, m])), n
        if n == 0:
            a.g['raw'].holds_fill(), b.g['raw'].holds_fill()


# ------------------------------------------------------------------------------------------------ K4
K4_OUT = (('rgb', 3), ('alpha', 1), ('depth', 1))
K4_DIAG = (('weights_on_rays', S0), ('rgb_on_rays', 3 * S0), ('cnl_xyz', 3), ('cnl_rgb', 3), ('cnl_weight', 1))


@pytest.mark.parametrize('cull_eps', [0.0, refs.K4_CULL_EPS])
@pytest.mark.parametrize('diag', [False, True], ids=['lean', 'diag'])
@pytest.mark.parametrize('S', [2, 21, 65, 512])
def test_composite(S, diag, cull_eps):
    """hnrf_composite_fwd with the five nullable outputs all null (and xyz null) or all given.  cull_eps > 0: the raw of
    every culled sample is left at the fill, so a kernel that interprets it computes something else under each fill.
    z_vals[p + 1] of the last sample of the last ray lies behind the input."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    R = R0
    c4 = refs.k4_problem(R, S, 'sparse')
    c4['mask'] = off_threshold(c4['mask'], cull_eps)
    culled = c4['mask'] < cull_eps
    if cull_eps:
        assert 0 < culled.sum() < R * S and (np.abs(c4['mask'] - cull_eps) > 1e-4).all()
    per = dict(K4_OUT + K4_DIAG, weights_on_rays=S, rgb_on_rays=3 * S)
    names = [k for k, _ in K4_OUT] + ([k for k, _ in K4_DIAG] if diag else [])
    cm = torch.from_numpy(culled.reshape(-1)).to(dev())

    def call(c):
        raw = c.put('raw', c4['raw'])
        c.i('raw', R * S, 4)[cm] = gb.as_i32(c.fill)                # culled samples never went through the MLPs
        c.orig['raw'] = c.g['raw'].interior_bytes().clone()
        outs = [c.new(k, 4 * R * per[k]) for k in names] + [None] * (0 if diag else 5)
        ok(lib.hnrf_composite_fwd(raw, c.put('mask', c4['mask']), c.put('z', c4['z']), c.put('rays_d', c4['rays_d']),
                                  c.put('xyz', c4['xyz']) if diag else None, c.put('bg', c4['bg']), R, S, cull_eps, *outs,
                                  _stream()), 'hnrf_composite_fwd')
    a, b = both(call)
    same(a, b, names)
    raw = T(c4['raw']).clone()
    raw.view(-1, 4)[cm] = 0.0                                     # (any defined value: culled samples' raw is not interpreted)
    want = ops.composite(raw, T(c4['mask']), T(c4['z']), T(c4['rays_d']), T(c4['xyz']), T(c4['bg']), diagnostics=diag,
                         cull_eps=cull_eps)
    for k in names:
        eq(a, k, want[k])


# ------------------------------------------------------------------------------------------------ baked samplers
GRID_N = 8                                                    # the minimum of both grids
BOX = (np.full(3, -1.0, F), np.full(3, 1.0, F))


@pytest.fixture(scope='module')
def grids(mlps):
    """The canonical grid and the offset grid at N = M = 8 over [-1, 1]^3, baked once (f32): dict(cnl, off) of f16
    (8, 8, 8, 4) device tensors."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    assert lib.hnrf_baked_grid_bytes(GRID_N) == GRID_N ** 3 * 8 and lib.hnrf_baked_grid_bytes(GRID_N - 1) == 0
    cnl = ops.bake_canonical(mlps['f32']['cnl'][0].clone(), T(BOX[0]), T(BOX[1]), GRID_N, 'f32')
    off = ops.bake_nonrigid(mlps['f32']['nr'][0].clone(), T(mlps['hann']), T(BOX[0]), T(BOX[1]), GRID_N, 'f32')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(cnl.float()).all()) and bool(torch.isfinite(off.float()).all())
    return dict(cnl=cnl, off=off)


def grid_args(c, grids, which):
    return [c.put(which + '_grid', grids[which]), GRID_N, c.put(which + '_bmin', BOX[0]), c.put(which + '_bmax', BOX[1])]


@pytest.mark.parametrize('P', [1, P0])
def test_baked_sample(grids, P):
    """hnrf_baked_sample and _sparse on the 4096-byte grid: points inside, outside (clamped) and a NaN coordinate."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    x = positions(P, 3) * 2
    if P > 8:
        x[5, 1] = np.nan
        assert (np.abs(x[~np.isnan(x).any(1)]) > 1).any() and (np.abs(x) < 1).all(1).any()
    box = T(BOX[0]), T(BOX[1])

    def dense(c):
        ok(lib.hnrf_baked_sample(c.put('xyz', x), *grid_args(c, grids, 'cnl'), P, c.new('raw', 16 * P), _stream()),
           'hnrf_baked_sample')
    a, b = both(dense)
    same(a, b, ['raw'])
    raw = ops.baked_sample(T(x), grids['cnl'], *box)
    eq(a, 'raw', raw)
    for n in [k for k in SPARSE_COUNTS if k <= P]:
        idx, count, m = listed(P, n)

        def sparse(c):
            ok(lib.hnrf_baked_sample_sparse(c.put('xyz', x), *grid_args(c, grids, 'cnl'), P, c.put('idx', idx),
                                            c.put('count', count), c.new('raw', 16 * P), _stream()), 'hnrf_baked_sample_sparse')
        a, b = both(sparse)
        same(a, b, ['raw'], rows=m, n_rows=P, row_bytes=16)
        assert torch.equal(bits(a.f('raw', P, 4)[m]), bits(raw[m])), n
        for c in (a, b):
            c.g['raw'].rows_hold_fill(~m, P, 16)


@pytest.mark.parametrize('lean', [False, True], ids=['diag', 'lean'])
@pytest.mark.parametrize('P', [1, P0])
def test_baked_warp_sample(grids, P, lean):
    """hnrf_baked_warp_sample and _sparse: xyz and offsets null and given; the sparse form writes raw, xyz and offsets at
    the listed samples only."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    x = positions(P, 4) * 2
    box = T(BOX[0]), T(BOX[1])
    names = ['raw'] + ([] if lean else ['xyz', 'offsets'])
    width = dict(raw=16, xyz=12, offsets=12)

    def outs(c):
        return [c.new('raw', 16 * P), None if lean else c.new('xyz', 12 * P), None if lean else c.new('offsets', 12 * P)]

    def dense(c):
        ok(lib.hnrf_baked_warp_sample(c.put('x', x), *grid_args(c, grids, 'off'), *grid_args(c, grids, 'cnl'), P, *outs(c),
                                      _stream()), 'hnrf_baked_warp_sample')
    a, b = both(dense)
    same(a, b, names)
    want = dict(zip(('raw', 'xyz', 'offsets'), ops.baked_warp_sample(T(x), (grids['off'],) + box, (grids['cnl'],) + box,
                                                                     want_xyz=True, want_offsets=True)))
    for k in names:
        eq(a, k, want[k])
    for n in [k for k in SPARSE_COUNTS if k <= P]:
        idx, count, m = listed(P, n)

        def sparse(c):
            ok(lib.hnrf_baked_warp_sample_sparse(c.put('x', x), *grid_args(c, grids, 'off'), *grid_args(c, grids, 'cnl'), P,
                                                 c.put('idx', idx), c.put('count', count), *outs(c), _stream()),
               'hnrf_baked_warp_sample_sparse')
        a, b = both(sparse)
        for k in names:
            same(a, b, [k], rows=m, n_rows=P, row_bytes=width[k])
            assert torch.equal(bits(a.f(k, P, width[k] // 4)[m]), bits(want[k][m])), (k, n)
            for c in (a, b):
                c.g[k].rows_hold_fill(~m, P, width[k])


# ------------------------------------------------------------------------------------------------ ray generation
RAYGEN_H, RAYGEN_W = 37, 53


def raygen_problem():
    """A 37 x 53 camera that sees the box in the middle of its image: some pixels hit, some miss, none grazes."""
    from humannerf_amd import scene
    K, E = refs._camera((2.0, 1.0, 3.0), (0, 0, 0), RAYGEN_H, RAYGEN_W, 40.0)
    mn, mx = refs.raygen_box()
    ro, rd = scene.get_rays_from_KRT(RAYGEN_H, RAYGEN_W, K, E[:3, :3], E[:3, 3])
    ro, rd = np.ascontiguousarray(ro.reshape(-1, 3), F), rd.reshape(-1, 3).astype(F).copy()
    bounds = np.stack([mn, mx])
    _, _, hit = scene.rays_intersect_3d_bbox(bounds, ro, rd)
    margin = refs.raygen_margin(bounds, ro, rd)
    return K, E, mn, mx, hit, margin


def raygen_call(lib, c, K, E, mn, mx, H, W, ws_bytes=None, misalign=0, ws=None):
    n = H * W
    need = lib.hnrf_gen_rays_workspace_bytes(H, W)
    ws_bytes = need if ws_bytes is None else ws_bytes
    if ws is not None:
        c.g['ws'], ws_bytes = ws, ws.nbytes
        assert need <= ws_bytes
    return lib.hnrf_gen_rays(c.put('Kinv', np.linalg.inv(K).astype(F)), c.put('R', E[:3, :3].astype(F)),
                             c.put('T', E[:3, 3].astype(F)), c.put('mn', mn), c.put('mx', mx), H, W, c.new('rays_o', 12 * n),
                             c.new('rays_d', 12 * n), c.new('near', 4 * n), c.new('far', 4 * n), c.new('ray_mask', n),
                             c.new('count', 4), c.g['ws'].ptr if ws is not None else c.new('ws', ws_bytes, misalign), ws_bytes,
                             _stream())


def test_gen_rays():
    """hnrf_gen_rays on a 37 x 53 image: the ray buffers' entries from *count on are not written, the mask is 1961 bytes
    and ends inside a word, the workspace is ceil(1961 / 256) ints."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    K, E, mn, mx, hit, margin = raygen_problem()
    H, W, n = RAYGEN_H, RAYGEN_W, RAYGEN_H * RAYGEN_W
    kept = int(hit.sum())
    assert 0 < kept < n and kept > 256 and kept % 256 and (margin > refs.RAYGEN_MARGIN).all()
    a, b = both(lambda c: ok(raygen_call(lib, c, K, E, mn, mx, H, W), 'hnrf_gen_rays'))
    # workspace A again, directly after another camera's call on it (every pixel hits: other block counts)
    K2, E2 = refs._camera((0.05, 0.1, 0.2), (0.4, 0.3, 1.0), H, W, 30.0)
    dirty, third = Case(gb.FILLS[0]), Case(gb.FILLS[0])
    ok(raygen_call(lib, dirty, K2, E2, mn, mx, H, W, ws=a.g['ws']), 'hnrf_gen_rays (the call in between)')
    ok(raygen_call(lib, third, K, E, mn, mx, H, W, ws=a.g['ws']), 'hnrf_gen_rays (after it)')
    dirty.done(), third.done()
    assert int(dirty.i('count')[0]) > kept
    want = ops.gen_rays(K, E, mn, mx, H, W)
    for c in (a, b, third):
        assert int(c.i('count')[0]) == kept
        assert np.array_equal(c.g['ray_mask'].view(torch.uint8).cpu().numpy().astype(bool), hit)
        for k, w in (('rays_o', 12), ('rays_d', 12), ('near', 4), ('far', 4)):
            c.g[k].rows_hold_fill(torch.arange(kept, n), n, w)
    rows = torch.arange(kept)
    for o in (b, third):
        same(a, o, ['ray_mask', 'count'])
        for k, w in (('rays_o', 12), ('rays_d', 12), ('near', 4), ('far', 4)):
            same(a, o, [k], rows=rows, n_rows=n, row_bytes=w)
    assert torch.equal(bits(a.f('rays_o', n, 3)[:kept]), bits(want['rays'][0]))
    assert torch.equal(bits(a.f('rays_d', n, 3)[:kept]), bits(want['rays'][1]))
    assert torch.equal(bits(a.f('near')[:kept]), bits(want['near'])) and torch.equal(bits(a.f('far')[:kept]), bits(want['far']))
    assert torch.equal(a.g['ray_mask'].view(torch.uint8).bool(), want['ray_mask'])


def test_gen_rays_refuses():
    """A workspace one byte short is HNRF_E_WORKSPACE, one at a 128-byte offset HNRF_E_ARG; nothing is written."""
    from humannerf_amd import _lib
    lib = _lib.load()
    K, E, mn, mx, _, _ = raygen_problem()
    need = lib.hnrf_gen_rays_workspace_bytes(RAYGEN_H, RAYGEN_W)
    assert need == 4 * 8
    for kw, rc in ((dict(ws_bytes=need - 1), E_WORKSPACE), (dict(misalign=128), E_ARG)):
        for fill in gb.FILLS:
            c = Case(fill)
            assert raygen_call(lib, c, K, E, mn, mx, RAYGEN_H, RAYGEN_W, **kw) == rc, (kw, lib.hnrf_last_error())
            c.done()
            for k in ('rays_o', 'rays_d', 'near', 'far', 'ray_mask', 'count', 'ws'):
                c.g[k].holds_fill()


# ================================================================================================ 3. entry-level workspaces
N_FRAME, CHUNK = R0, 15                                       # chunks of 15, 15 and 7 rays: both slots alternate, the last is ragged
H_FRAME = 3
CULL = 0.3
LEAN = ('rgb', 'alpha', 'depth')
HEAD_KEYS = ('rgb', 'alpha', 'depth', 'weights_on_rays', 'rgb_on_rays', 'cnl_xyz', 'cnl_rgb', 'cnl_weight')
ALL_KEYS = HEAD_KEYS + ('xyz_on_rays', BMW, 'offsets')


@pytest.fixture(scope='module')
def frame_problem():
    """K1's inputs of the frame (24 bones: the shared entries classify inside K1) and of the larger call that dirties the
    workspace in between -- more rays and more samples in chunks of the same 315 samples, so that it runs in the same
    workspace --, with what the fp64 K1 reference says about both."""
    pr = refs.k1_problem(24, 16, S0, N_FRAME)
    big = refs.k1_problem(24, 16, 35, 50, seed=3)
    r = refs.ref_k1(pr, True)
    wsum, x = r['wsum'].numpy(), r['x'].abs().amax(1).numpy()
    return dict(pr=pr, big=big, big_chunk=9, wsum=wsum.reshape(N_FRAME, S0), xmax=x.reshape(N_FRAME, S0))


def frame_conditions(fp, form):
    """The issue's conditions on the inputs, from the fp64 K1 reference, with a margin from every threshold."""
    wsum, xmax = fp['wsum'], fp['xmax']
    if form.get('share'):
        shared, live = wsum == 0, xmax > 1e-3                     # x_skel = 0 without any weight; a body-sized one is live
        assert (shared | live).all()
        per_chunk = [(shared[r:r + CHUNK].any(), live[r:r + CHUNK].any()) for r in range(0, N_FRAME, CHUNK)]
        assert any(s and l for s, l in per_chunk), per_chunk
    if form.get('cull'):
        assert (np.abs(wsum - form['cull']) > 1e-4).all()
        assert 0 < (wsum < form['cull']).sum() < wsum.size


def key_shapes(S, B, diag):
    from humannerf_amd import ops
    return ops.output_shapes(S, B, diag)


def sync_args(side):
    """(side stream, its five events) as the frame entries take them, or (None, None)."""
    from humannerf_amd import ops
    if not side:
        return None, None
    s, evs = ops._frame_streams(dev())
    return s.cuda_stream, (ctypes.c_void_p * 5)(*[e.cuda_event for e in evs])


def entry_need(lib, kind, rows, S, H):
    if kind.startswith('rays'):
        return lib.hnrf_render_workspace_bytes(rows, S)
    return {'frame': lambda: lib.hnrf_render_frame_workspace_bytes(rows, S),
            'frame_baked': lambda: lib.hnrf_render_frame_workspace_bytes(rows, S),
            'frame_baked_nr': lambda: lib.hnrf_render_frame_workspace_bytes(rows, S),
            'frame_shared': lambda: lib.hnrf_render_frame_shared_workspace_bytes(rows, S),
            'frame_heads': lambda: lib.hnrf_render_frame_heads_workspace_bytes(rows, S, H),
            'frame_heads_shared': lambda: lib.hnrf_render_frame_heads_shared_workspace_bytes(rows, S, H)}[kind]()


def call_entry(lib, kind, c, pr, chunk, form, mlps, grids, ws=None, ws_bytes=None, misalign=0):
    """One call of a render entry with every buffer in case ``c``; ``ws``: a GuardedBuffer to run in instead of a fresh
    workspace of exactly the stated size.  Returns (rc, names of the output buffers)."""
    from humannerf_amd import ops
    mode, diag, cull, H = form.get('mode', 'f16x3'), form.get('diag', False), form.get('cull', 0.0), form.get('H', 0)
    N, S, B, G = pr['R'], pr['S'], pr['B'], pr['G']
    heads, share, frame = 'heads' in kind, 'shared' in kind, kind.startswith('frame')
    ptrs = k1_inputs(c, pr, True)
    if kind.endswith('baked_nr'):
        ptrs += grid_args(c, grids, 'off')
    elif form.get('nr', True):
        ptrs += [c.put('hann', mlps['hann']), c.packed('nr', mlps[mode]['nr'])]
    else:                                                         # cfg.ignore_non_rigid_motions: xyz = x_skel, offsets = 0
        ptrs += [None, None]
    if 'baked' in kind:
        ptrs += grid_args(c, grids, 'cnl')
    else:
        ptrs += [c.packed('cnl', mlps[mode]['heads', H] if heads else mlps[mode]['cnl'])]
    ptrs += [c.put('bg', np.array([255., 128., 0.], F))]
    rows = min(chunk, N) if frame else N
    need = entry_need(lib, kind, rows, S, H)
    assert need > 0
    if ws is None:
        ws_bytes = need if ws_bytes is None else ws_bytes
        c.new('ws', ws_bytes, misalign)
    else:
        c.g['ws'] = ws
        ws_bytes = ws.nbytes
        assert need <= ws_bytes
    shapes = key_shapes(S, B, diag and frame)
    names = []

    def out(k):
        if k not in shapes:
            return None
        per = int(np.prod(shapes[k], dtype=np.int64)) * 4 * N
        if heads and k in HEAD_KEYS:
            names.extend('%s.%d' % (k, h) for h in range(H))
            return (ctypes.c_void_p * H)(*[c.new('%s.%d' % (k, h), per) for h in range(H)])
        names.append(k)
        return c.new(k, per)
    dims = [ops._mode_arg(mode), float(cull), N, S, B, G]
    if not frame:
        rc = getattr(lib, 'hnrf_render_%s_fwd' % kind)(*ptrs, *dims, c.g['ws'].ptr, ws_bytes, *[out(k) for k in LEAN], None, None,
                                                       _stream())
        return rc, names
    side, events = sync_args(form.get('side', False))
    nchunk = -(-N // chunk)
    live = [c.new('live_counts', 4 * nchunk)] if share else []
    rc = getattr(lib, 'hnrf_render_%s_fwd' % kind)(*ptrs, *dims, chunk, *([H] if heads else []), c.g['ws'].ptr, ws_bytes,
                                                   *[out(k) for k in ALL_KEYS], *live, side, events, None, _stream())
    return rc, names


def ops_entry(kind, pr, chunk, form, mlps, grids):
    """The same call through the ops wrapper on allocator-provided buffers: dict name -> tensor (heads: 'key.h')."""
    from humannerf_amd import ops
    mode, diag, cull, H = form.get('mode', 'f16x3'), form.get('diag', False), form.get('cull', 0.0), form.get('H', 0)
    B = pr['B']
    box = T(BOX[0]), T(BOX[1])
    k1 = (T(pr['rays_o']), T(pr['rays_d']), T(pr['near']), T(pr['far']), T(pr['t_rand']), T(pr['Rs']), T(pr['Ts']),
          T(pr['vol'][:B]), T(pr['bmin']), T(pr['bscale']))
    nr_baked = kind.endswith('baked_nr')
    mid = (None, None) if nr_baked or not form.get('nr', True) else (T(mlps['hann']), mlps[mode]['nr'][0].clone())
    cnl = None if 'baked' in kind else (mlps[mode]['heads', H] if 'heads' in kind else mlps[mode]['cnl'])[0].clone()
    args = k1 + mid + (cnl, T(np.array([255., 128., 0.], F)))
    kw = {}
    if 'baked' in kind:
        kw['baked'] = (grids['cnl'],) + box
    if nr_baked:
        kw['baked_nr'] = (grids['off'],) + box
    if kind.startswith('rays'):
        out = ops.render_rays(*args, pr['S'], mode, cull_eps=cull, **kw)
    elif 'heads' in kind:
        out, _ = ops.render_frame_heads(*args, pr['S'], chunk, H, mode, diagnostics=diag, cull_eps=cull, overlap=False,
                                        share_log=[] if 'shared' in kind else None)
        flat = {}
        for k, v in out.items():
            if k in HEAD_KEYS:
                flat.update({'%s.%d' % (k, h): v[h] for h in range(H)})
            else:
                flat[k] = v[0] if isinstance(v, list) else v
        out = flat
    else:
        out, _ = ops.render_frame(*args, pr['S'], chunk, mode, diagnostics=diag, cull_eps=cull, overlap=False,
                                  share_log=[] if 'shared' in kind else None, **kw)
    torch.cuda.synchronize()
    return out


def other_form(kind, form):
    """The form of the larger call in between: the other cull setting where the entry has one, the other head count."""
    o = dict(form, side=False)
    if not form.get('diag') and 'shared' not in kind:
        o['cull'] = 0.0 if form.get('cull') else CULL
    if form.get('H'):
        o['H'] = 2
    return o


def three_runs(kind, form, fp, mlps, grids):
    """Fill A, fill B, then workspace A again directly after a larger call on it: guards, outputs bit-equal across the
    three runs and to the ops wrapper."""
    lib = lib_all()
    frame = kind.startswith('frame')
    frame_conditions(fp, dict(form, share='shared' in kind))
    pr, big = fp['pr'], fp['big']
    chunk, big_chunk = (CHUNK, fp['big_chunk']) if frame else (N_FRAME, 0)
    if not frame:                                                 # one chunk: the larger call has more rays of fewer samples
        big = refs.k1_problem(24, 16, 7, 111, seed=3)
        assert big['R'] * big['S'] == N_FRAME * S0
    runs = []
    for fill in gb.FILLS:
        c = Case(fill)
        rc, names = call_entry(lib, kind, c, pr, chunk, form, mlps, grids)
        ok(rc, kind)
        runs.append(c.done())
    a, b = runs
    dirty = Case(gb.FILLS[0])
    rc, _ = call_entry(lib, kind, dirty, big, big_chunk, other_form(kind, form), mlps, grids, ws=a.g['ws'])
    ok(rc, kind + ' (the larger call)')
    third = Case(gb.FILLS[0])
    rc, _ = call_entry(lib, kind, third, pr, chunk, form, mlps, grids, ws=a.g['ws'])
    ok(rc, kind + ' (after the larger call)')
    dirty.done(), third.done()
    same(a, b, names)
    same(a, third, names)
    want = ops_entry(kind, pr, chunk, form, mlps, grids)
    for n in names:
        eq(a, n, want[n])
    if 'live_counts' in a.g:
        print('%s %s live_counts %s of %d samples per whole chunk' % (kind, form, a.i('live_counts').tolist(), CHUNK * S0))


FRAME_FORMS = [dict(), dict(cull=CULL, side=True), dict(diag=True, side=True), dict(diag=True, mode='f32')]
SHARED_FORMS = [dict(), dict(side=True), dict(diag=True), dict(diag=True, side=True)]
form_id = lambda f: '-'.join('%s%s' % (k, '' if v is True else v) for k, v in sorted(f.items())) or 'lean'


@pytest.mark.parametrize('form', FRAME_FORMS, ids=form_id)
@pytest.mark.parametrize('kind', ['frame', 'frame_baked', 'frame_baked_nr'])
def test_frame_entries(kind, form, frame_problem, mlps, grids):
    """hnrf_render_frame_fwd, _baked_fwd, _baked_nr_fwd: lean and diagnostic outputs, cull_eps 0 and > 0, side stream
    null and given; a workspace of exactly hnrf_render_frame_workspace_bytes(15, 21)."""
    three_runs(kind, form, frame_problem, mlps, grids)


@pytest.mark.parametrize('kind,form', [('frame', dict(nr=False, diag=True, side=True)), ('frame', dict(nr=False, cull=CULL)),
                                       ('frame_baked', dict(nr=False, diag=True)), ('rays', dict(nr=False))],
                         ids=lambda v: v if isinstance(v, str) else form_id(v))
def test_entries_without_the_nonrigid_mlp(kind, form, frame_problem, mlps, grids):
    """nr_packed == NULL: the diagnostic form copies x_skel into xyz_on_rays and clears offsets, chunk by chunk, with
    byte counts of its own."""
    three_runs(kind, form, frame_problem, mlps, grids)


@pytest.mark.parametrize('form', SHARED_FORMS, ids=form_id)
def test_frame_shared_entry(form, frame_problem, mlps, grids):
    """hnrf_render_frame_shared_fwd: the representative slot behind the two chunk workspaces."""
    three_runs('frame_shared', form, frame_problem, mlps, grids)


@pytest.mark.parametrize('form', [dict(H=H_FRAME), dict(H=H_FRAME, cull=CULL, side=True), dict(H=H_FRAME, diag=True, side=True)],
                         ids=form_id)
def test_frame_heads_entry(form, frame_problem, mlps, grids):
    """hnrf_render_frame_heads_fwd, H = 3: one set of head planes behind the chunk workspaces."""
    three_runs('frame_heads', form, frame_problem, mlps, grids)


@pytest.mark.parametrize('form', [dict(H=H_FRAME), dict(H=H_FRAME, side=True), dict(H=H_FRAME, diag=True, side=True)], ids=form_id)
def test_frame_heads_shared_entry(form, frame_problem, mlps, grids):
    """hnrf_render_frame_heads_shared_fwd, H = 3: the slot and two sets of head planes."""
    three_runs('frame_heads_shared', form, frame_problem, mlps, grids)


@pytest.mark.parametrize('form', [dict(), dict(cull=CULL), dict(mode='f32')], ids=form_id)
@pytest.mark.parametrize('kind', ['rays', 'rays_baked', 'rays_baked_nr'])
def test_ray_chunk_entries(kind, form, frame_problem, mlps, grids):
    """hnrf_render_rays_fwd, _baked_fwd, _baked_nr_fwd on one chunk of 37 rays."""
    three_runs(kind, form, frame_problem, mlps, grids)


REFUSED = [('rays', dict()), ('rays_baked', dict()), ('rays_baked_nr', dict()), ('frame', dict(diag=True)),
           ('frame_baked', dict()), ('frame_baked_nr', dict()), ('frame_shared', dict()), ('frame_heads', dict(H=H_FRAME)),
           ('frame_heads_shared', dict(H=H_FRAME, diag=True))]


@pytest.mark.parametrize('kind,form', REFUSED, ids=[k for k, _ in REFUSED])
def test_entries_refuse_short_and_misaligned_workspaces(kind, form, frame_problem, mlps, grids):
    """need - 1 bytes: HNRF_E_WORKSPACE; the stated size at a 128-byte offset: HNRF_E_ARG.  Outputs and workspace keep
    their fill."""
    lib = lib_all()
    pr = frame_problem['pr']
    chunk = CHUNK if kind.startswith('frame') else N_FRAME
    need = entry_need(lib, kind, min(chunk, N_FRAME), S0, form.get('H', 0))
    for kw, want in ((dict(ws_bytes=need - 1), E_WORKSPACE), (dict(misalign=128), E_ARG)):
        for fill in gb.FILLS:
            c = Case(fill)
            rc, names = call_entry(lib, kind, c, pr, chunk, form, mlps, grids, **kw)
            assert rc == want, (kind, kw, rc, lib.hnrf_last_error())
            c.done()
            for n in names + ['ws'] + (['live_counts'] if 'shared' in kind else []):
                c.g[n].holds_fill()


# ------------------------------------------------------------------------------------------------ early termination
TERM_R, TERM_S, TERM_EPS, TERM_BIAS = 13, 70, 1e-2, 6.0        # slabs of 32, 32 and 6 samples; 13 rays: a ragged half-wave block


@pytest.fixture(scope='module')
def term_setup():
    """refs.term_problem with its own weights (the bias on the sigma head decides where the rays saturate), packed per
    mode, and what the fp64 references say: which rays are dead before the last slab."""
    from humannerf_amd import _lib, ops
    from oracle import oracle
    lib = _lib.load()
    pr = refs.term_problem(TERM_R, TERM_S, TERM_BIAS)
    r = refs.ref_k1(dict(pr, near=pr['near'][:, None], far=pr['far'][:, None]), True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    st = {n + '.weight': t(w) for n, w in zip(CNL_NAMES + NR_NAMES, pr['cw'] + pr['nw'])}
    st.update({n + '.bias': t(b) for n, b in zip(CNL_NAMES + NR_NAMES, pr['cb'] + pr['nb'])})
    xyz, _ = oracle.non_rigid_mlp(st, oracle.hann_pe(r['x'], t(pr['hann'])), t(pr['cond'])[None], r['x'])
    raw = oracle.canonical_mlp(st, oracle.fourier_pe(xyz, 10)).reshape(TERM_R, TERM_S, 4)
    mask = r['wsum'].reshape(TERM_R, TERM_S)
    packs = {}
    for mode in MODES:
        packs[mode] = {'cnl': _image(lib, ops.canonical_pack([T(w) for w in pr['cw']], [T(b) for b in pr['cb']], mode),
                                     'canonical', mode),
                       'nr': _image(lib, ops.nonrigid_pack([T(w) for w in pr['nw']], [T(b) for b in pr['nb']], T(pr['cond']), mode),
                                    'nonrigid', mode)}
    torch.cuda.synchronize()
    return dict(pr=pr, raw=raw, mask=mask, z=r['z'], packs=packs)


def term_call(lib, c, pr, packs, mode, cull, ws=None, ws_bytes=None, misalign=0):
    from humannerf_amd import ops
    R, S = pr['R'], pr['S']
    need = lib.hnrf_render_term_workspace_bytes(R, S)
    if ws is None:
        ws_bytes = need if ws_bytes is None else ws_bytes
        c.new('ws', ws_bytes, misalign)
    else:
        c.g['ws'], ws_bytes = ws, ws.nbytes
        assert need <= ws_bytes
    return lib.hnrf_render_rays_term_fwd(*k1_inputs(c, pr, True), c.put('hann', pr['hann']), c.packed('nr', packs[mode]['nr']),
                                         c.packed('cnl', packs[mode]['cnl']), c.put('bg', pr['bg']), ops._mode_arg(mode),
                                         float(cull), TERM_EPS, R, S, pr['B'], pr['G'], c.g['ws'].ptr, ws_bytes,
                                         c.new('rgb', 12 * R), c.new('alpha', 4 * R), c.new('depth', 4 * R),
                                         c.new('evaluated', 4), _stream())


@pytest.mark.parametrize('cull', [0.0, CULL])
@pytest.mark.parametrize('mode', MODES)
def test_termination_entry(term_setup, mode, cull):
    """hnrf_render_rays_term_fwd, R = 13, S = 70: a workspace of exactly hnrf_render_term_workspace_bytes, three runs as
    the frame entries.  From the fp64 references: at least one ray is dead before the last slab and one is alive, none
    within a relative 1e-2 of the threshold at a slab entry; with cull_eps both culled and kept samples exist."""
    from humannerf_amd import _lib, ops
    lib = _lib.load()
    s, pr = term_setup, term_setup['pr']
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    walk = refs.ref_slab_walk(s['raw'], s['mask'], s['z'], t(pr['rays_d']), t(pr['bg']), cull, TERM_EPS)
    ev = s['mask'] >= cull
    a_full = (1.0 - torch.exp(-torch.relu(s['raw'][..., 3]) * torch.cat(
        [s['z'][:, 1:] - s['z'][:, :-1], torch.full_like(s['z'][:, :1], 1e10)], -1) * t(pr['rays_d']).norm(dim=-1, keepdim=True))) * s['mask']
    T_last = torch.cumprod(1.0 - torch.where(ev, a_full, torch.zeros_like(a_full)) + 1e-10, 1)[:, 63]   # before the last slab
    assert float(walk['closeness'].min()) > 1e-2
    assert bool((T_last < TERM_EPS).any()) and bool((T_last >= TERM_EPS).any()), T_last
    if cull:
        assert 0 < int((~ev).sum()) < ev.numel() and float((s['mask'] - cull).abs().min()) > 1e-4
    packs = s['packs']
    runs = []
    for fill in gb.FILLS:
        c = Case(fill)
        ok(term_call(lib, c, pr, packs, mode, cull), 'hnrf_render_rays_term_fwd')
        runs.append(c.done())
    a, b = runs
    big = refs.term_problem(14, 65, 2.5, seed=5)                  # 910 samples as well, another ray count, a thin medium
    dirty, third = Case(gb.FILLS[0]), Case(gb.FILLS[0])
    ok(term_call(lib, dirty, big, packs, mode, 0.0 if cull else CULL, ws=a.g['ws']), 'term (the larger call)')
    ok(term_call(lib, third, pr, packs, mode, cull, ws=a.g['ws']), 'term (after the larger call)')
    dirty.done(), third.done()
    same(a, b, LEAN)
    same(a, third, LEAN)
    want = ops.render_rays_term(T(pr['rays_o']), T(pr['rays_d']), T(pr['near']), T(pr['far']), T(pr['t_rand']), T(pr['Rs']),
                                T(pr['Ts']), T(pr['vol'][:24]), T(pr['bmin']), T(pr['bscale']), T(pr['hann']),
                                packs[mode]['nr'][0].clone(), packs[mode]['cnl'][0].clone(), T(pr['bg']), TERM_S, mode,
                                term_eps=TERM_EPS, cull_eps=cull)
    torch.cuda.synchronize()
    for k in LEAN:
        eq(a, k, want[k])
    print('term %s cull %g: evaluated %s of %d (fp64 walk: %d)' % (mode, cull, [int(c.i('evaluated')[0]) for c in (a, b, third)],
                                                                  TERM_R * TERM_S, walk['evaluated']))


def test_termination_entry_refuses(term_setup):
    from humannerf_amd import _lib
    lib = _lib.load()
    pr, packs = term_setup['pr'], term_setup['packs']
    need = lib.hnrf_render_term_workspace_bytes(TERM_R, TERM_S)
    for kw, want in ((dict(ws_bytes=need - 1), E_WORKSPACE), (dict(misalign=128), E_ARG)):
        for fill in gb.FILLS:
            c = Case(fill)
            assert term_call(lib, c, pr, packs, 'f16x3', 0.0, **kw) == want, (kw, lib.hnrf_last_error())
            c.done()
            for n in LEAN + ('evaluated', 'ws'):
                c.g[n].holds_fill()


# ------------------------------------------------------------------------------------------------ lattice entries
# hnrf_density_grid and the two bakes walk the N^3 lattice in chunks of kLatticeChunk = 2^21 points
# (humannerf_amd/csrc/hnrf_common.h): 128^3 = 2^21 is still one launch, N = 129 is the smallest that needs two.
LATTICE_CHUNK = 1 << 21
N_TWO_LAUNCHES = 129
assert (N_TWO_LAUNCHES - 1) ** 3 <= LATTICE_CHUNK < N_TWO_LAUNCHES ** 3 < 2 * LATTICE_CHUNK


def lattice_call(lib, which, c, mlps, mode, N, ws_bytes=None, misalign=0, ws=None):
    from humannerf_amd import ops
    need = getattr(lib, 'hnrf_%s_workspace_bytes' % which)(N)
    assert need > 0
    if ws is None:
        ws_bytes = need if ws_bytes is None else ws_bytes
        c.new('ws', ws_bytes, misalign)
    else:
        c.g['ws'], ws_bytes = ws, ws.nbytes
        assert need <= ws_bytes
    m, box = ops._mode_arg(mode), [c.put('bmin', BOX[0]), c.put('bmax', BOX[1])]
    n3 = N ** 3
    if which == 'density_grid':
        pr = refs.k1_problem(24, 16, 2, 1)
        return lib.hnrf_density_grid(c.packed('cnl', mlps[mode]['cnl']), m, c.put('vol', pr['vol'][:24]), 24, 16, *box,
                                     c.put('bscale', np.ones(3, F)), N, c.g['ws'].ptr, ws_bytes, c.new('density', 4 * n3),
                                     c.new('sigma', 4 * n3), c.new('fg', 4 * n3), _stream())
    sat = c.put('saturated', np.zeros(1, np.int32))
    del c.orig['saturated']                                       # (a counter that is added to)
    if which == 'bake_canonical':
        return lib.hnrf_bake_canonical(c.packed('cnl', mlps[mode]['cnl']), m, *box, N, c.g['ws'].ptr, ws_bytes,
                                       c.new('grid', 8 * n3), sat, _stream())
    return lib.hnrf_bake_nonrigid(c.packed('nr', mlps[mode]['nr']), c.put('hann', mlps['hann']), m, *box, N, c.g['ws'].ptr,
                                  ws_bytes, c.new('grid', 8 * n3), sat, _stream())


def ops_lattice(which, mlps, mode, N):
    from humannerf_amd import ops
    box = T(BOX[0]), T(BOX[1])
    if which == 'density_grid':
        pr = refs.k1_problem(24, 16, 2, 1)
        vol = T(np.concatenate([pr['vol'][:24], np.zeros_like(pr['vol'][:1])]))       # (the wrapper takes B + 1 channels)
        d, s, f = ops.density_grid(mlps[mode]['cnl'][0].clone(), vol, *box, T(np.ones(3, F)), N, mode, want_parts=True)
        out = dict(density=d, sigma=s, fg=f)
    elif which == 'bake_canonical':
        g, sat = ops.bake_canonical(mlps[mode]['cnl'][0].clone(), *box, N, mode, want_saturated=True)
        out = dict(grid=g.view(torch.int32), saturated=sat)
    else:
        g, sat = ops.bake_nonrigid(mlps[mode]['nr'][0].clone(), T(mlps['hann']), *box, N, mode, want_saturated=True)
        out = dict(grid=g.view(torch.int32), saturated=sat)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('mode,N', [('f32', GRID_N), ('f16x3', GRID_N), ('f16x3', N_TWO_LAUNCHES)])
@pytest.mark.parametrize('which', ['density_grid', 'bake_canonical', 'bake_nonrigid'])
def test_lattice_entries(which, mode, N, mlps):
    """hnrf_density_grid, hnrf_bake_canonical, hnrf_bake_nonrigid at N = 8 (one chunk) and N = 129 (two launches, the
    second of 49 537 points), in a workspace of exactly the stated size; the third run follows a call of the other
    resolution on the same workspace."""
    from humannerf_amd import _lib
    lib = _lib.load()
    names = ('density', 'sigma', 'fg') if which == 'density_grid' else ('grid', 'saturated')
    runs = []
    for fill in gb.FILLS:
        c = Case(fill)
        ok(lattice_call(lib, which, c, mlps, mode, N), which)
        runs.append(c.done())
    a, b = runs
    same(a, b, names)
    if N > GRID_N:                                                # the other resolution fits this workspace
        dirty, third = Case(gb.FILLS[0]), Case(gb.FILLS[0])
        ok(lattice_call(lib, which, dirty, mlps, mode, 31, ws=a.g['ws']), which + ' (the call in between)')
        ok(lattice_call(lib, which, third, mlps, mode, N, ws=a.g['ws']), which + ' (after it)')
        dirty.done(), third.done()
        same(a, third, names)
    want = ops_lattice(which, mlps, mode, N)
    for n in names:
        eq(a, n, want[n])


@pytest.mark.parametrize('which', ['density_grid', 'bake_canonical', 'bake_nonrigid'])
def test_lattice_entries_refuse(which, mlps):
    from humannerf_amd import _lib
    lib = _lib.load()
    need = getattr(lib, 'hnrf_%s_workspace_bytes' % which)(GRID_N)
    names = ('density', 'sigma', 'fg') if which == 'density_grid' else ('grid',)
    for kw, want in ((dict(ws_bytes=need - 1), E_WORKSPACE), (dict(misalign=128), E_ARG)):
        for fill in gb.FILLS:
            c = Case(fill)
            assert lattice_call(lib, which, c, mlps, 'f16x3', GRID_N, **kw) == want, (kw, lib.hnrf_last_error())
            c.done()
            for n in names + ('ws',):
                c.g[n].holds_fill()
