"""Where the post-processing kernels write and read: the entries either side of the path -- the sections image
pre-processing, mesh extraction, rasteriser, LPIPS and image metrics of include/hnrf.h and every entry of hnrf_cloud.h,
hnrf_video.h, hnrf_segment.h, hnrf_geometry.h, hnrf_normals.h and hnrf_skin.h -- under the five assertions of
tests/test_gpu_buffer_bounds.py.  Every input, output, packed image and workspace of every call sits in a guarded buffer
(tests/guarded_buffers.py) of EXACTLY the size the header states or the ``*_bytes`` function returns, the call runs once
under each of the two fills, and

  (a) every guard is intact,
  (b) every output byte the header calls written is equal between the two fills,
  (c) it is bit-equal to what the entry's ops wrapper returns for the same inputs on allocator-provided buffers,
  (d) what the header calls not written still holds the fill (rows past a count, the bytes of a stream behind its
      length, every output under a raised status word or of a refused call),
  (e) every input holds what it held (Case.done does (a) and (e)).

Every entry with a ``*_workspace_bytes``: a call directly after a call of another shape in the same workspace equals a
fresh one; a workspace one byte short is HNRF_E_WORKSPACE, one misaligned by 4 bytes HNRF_E_ARG, and either way every
output and the workspace keep the fill.  The guards are 256 KiB: one LPIPS output tile is 64 KiB (256 pixels x 64
channels x 4 bytes), so a store one tile out would pass a 64 KiB guard only at its very edge.  None of these entries
uses float atomics: every comparison is on bits.  The values themselves are checked elsewhere (the files named after
each module); the cases are those of tests/aux_bounds_cases.py, which tests/test_aux_bounds_cases_cpu.py holds to the
numpy twins.  The C entries are called through humannerf_amd._lib with raw pointers.  Needs an MI355X: ``pytest -m gpu``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import aux_bounds_cases as ac
from tests import guarded_buffers as gb
from tests import guarded_case
from tests.guarded_case import Case, T, _stream, dev, eqb, ok, same

pytestmark = pytest.mark.gpu

GUARD = 256 * 1024
E_ARG, E_WORKSPACE = -1, -4
F = np.float32


def both(fn):
    """guarded_case.both between 256 KiB guards; fn returns the entry's return code, and one that is not 0 raises."""
    return guarded_case.both(fn, GUARD, check=True)


@functools.lru_cache(maxsize=None)
def lib():
    from humannerf_amd import _lib
    _lib.load_all(), _lib.load_late(), _lib.load_open()
    return _lib.load()


class Pre:
    """A Case seen through a name prefix: the buffers of a second call beside the first one's, one workspace for both."""

    def __init__(self, case, tag):
        self.case, self.tag = case, tag

    def put(self, name, a):
        return self.case.put(self.tag + name, a)

    def new(self, name, nbytes, misalign=0):
        return self.case.new(self.tag + name, nbytes, misalign)


def workspace(c, need, short=0, misalign=0, name='ws'):
    """(pointer, bytes) of the call's workspace: a buffer of exactly ``need`` bytes (``misalign``: moved off its
    alignment), or the one the case holds already; ``short``: that many bytes fewer are stated."""
    case = c.case if isinstance(c, Pre) else c
    if name not in case.g:
        case.new(name, need, misalign)
    g = case.g[name]
    assert need > 0 and g.nbytes >= need
    return g.ptr, g.nbytes - short


def check_refusals(run, outs, ws='ws'):
    """run(case, short=..., misalign=...) -> the entry's return code.  One byte short: HNRF_E_WORKSPACE; misaligned by
    4 bytes: HNRF_E_ARG; the outputs and the workspace keep the fill either way."""
    for kw, code in ((dict(short=1), E_WORKSPACE), (dict(misalign=4), E_ARG)):
        for fill in gb.FILLS:
            c = Case(fill, GUARD)
            rc = run(c, **kw)
            assert rc == code, (kw, rc, lib().hnrf_last_error())
            c.done()
            for n in list(outs) + [ws]:
                c.g[n].holds_fill()


def check_reuse(first, second, outs, need, ws='ws'):
    """``second`` directly after ``first`` (another shape) in one workspace of ``need`` bytes gives the bytes of
    ``second`` in a fresh workspace.  outs: {name: bytes to compare, None = all}."""
    fresh = both(second)
    for fill, alone in zip(gb.FILLS, fresh):
        c = Case(fill, GUARD)
        c.new(ws, need)
        ok(first(Pre(c, 'a_')) or 0, 'first call')
        ok(second(Pre(c, 'b_')) or 0, 'second call')
        c.done()
        for n, nbytes in outs.items():
            x, y = c.g['b_' + n].interior_bytes(), alone.g[n].interior_bytes()
            assert torch.equal(x[:nbytes], y[:nbytes]), n


def held(cases, names):
    for c in cases:
        for n in names:
            c.g[n].holds_fill()


# ================================================================================================ image pre-processing
@pytest.mark.parametrize('name', list(ac.UNDISTORT_CASES))
def test_undistort_image(name):
    """hnrf_undistort_image: src and dst of exactly H W C bytes (105, 5120 and 36: odd byte counts), cam [9] and
    ir [n_stripes][9] doubles; taps outside the image are constant 0 and read nothing."""
    from humannerf_amd import ops
    k = ac.undistort_case(name)
    H, W, C = k['img'].shape

    def call(c):
        return lib().hnrf_undistort_image(c.put('src', k['img']), H, W, C, c.put('cam', k['cam']), c.put('ir', k['ir']),
                                          k['n_stripes'], k['rows'], c.new('dst', H * W * C), _stream())
    a, b = both(call)
    same(a, b, ['dst'])
    eqb(a, 'dst', ops.undistort_image(T(k['img']), k['K'], k['D']))
    assert a.g['cam'].nbytes == 72 and a.g['ir'].nbytes == 72 * k['n_stripes']


@pytest.mark.parametrize('whole', [False, True], ids=['windows', 'whole'])
@pytest.mark.parametrize('scale', ac.COMPOSITE_SCALES)
def test_composite_windows(scale, whole):
    """hnrf_composite_windows: six 4 x 4 windows that touch all four borders (clamped taps) or one window of the whole
    image; the tables have exactly Wd / Hd rows."""
    from humannerf_amd import ops
    k = ac.composite_case(scale, whole)
    Hs, Ws = ac.COMPOSITE_SRC
    n = len(k['wins'])

    def call(c):
        t = [0, 0, 0, 0] if k['tables'] is None else [c.put(nm, a) for nm, a in zip(('xofs', 'xw', 'yofs', 'yw'), k['tables'])]
        return lib().hnrf_composite_windows(c.put('orig', k['orig']), c.put('alpha', k['alpha']), Hs, Ws, c.put('bg', k['bg']),
                                            int(k['tables'] is not None), *t, k['Hd'], k['Wd'], c.put('win', k['wins']), n,
                                            k['ph'], k['pw'], c.new('out', n * k['ph'] * k['pw'] * 12), _stream())
    a, b = both(call)
    same(a, b, ['out'])
    eqb(a, 'out', ops.composite_windows(T(k['orig']), T(k['alpha']), T(k['bg']), k['wins'], k['ph'], k['pw'], scale=scale))


@pytest.mark.parametrize('case', ac.MASK_CASES, ids=str)
def test_resize_mask(case):
    """hnrf_resize_mask, channel 2: the last byte of the last pixel is the last byte of the buffer."""
    from humannerf_amd import ops
    k = ac.mask_case(*case)
    Hs, Ws = case[0]

    def call(c):
        t = [0, 0, 0, 0] if k['tables'] is None else [c.put(nm, a) for nm, a in zip(('xofs', 'xw', 'yofs', 'yw'), k['tables'])]
        return lib().hnrf_resize_mask(c.put('alpha', k['alpha']), Hs, Ws, ac.MASK_CHANNEL, k['mode'], *t, k['Hd'], k['Wd'],
                                      c.new('out', k['Hd'] * k['Wd'] * 4), _stream())
    a, b = both(call)
    same(a, b, ['out'])
    eqb(a, 'out', ops.resize_mask(T(k['alpha']), k['scale'], channel=ac.MASK_CHANNEL))


# ===================================================================================================== mesh extraction
def mesh_need(N):
    return lib().hnrf_mesh_workspace_bytes(N)


def run_mesh_count(c, k, short=0, misalign=0):
    ws, nb = workspace(c, mesh_need(k['N']), short, misalign)
    return lib().hnrf_mesh_count(c.put('d', k['d']), k['N'], k['level'], ws, nb, c.new('counts', 16), _stream())


def run_mesh(c, k, drop=0, short=0, misalign=0):
    """hnrf_mesh_count, the counts read back, hnrf_mesh_emit into verts / faces of V - drop / F - drop rows."""
    base = c.case if isinstance(c, Pre) else c
    tag = c.tag if isinstance(c, Pre) else ''
    rc = run_mesh_count(c, k)
    if rc:
        return rc
    torch.cuda.synchronize()
    V, F_ = (int(v) for v in base.i64(tag + 'counts'))
    base.VF = (V, F_)
    nv, nf = max(V - drop, 0), max(F_ - drop, 0)
    ws, nb = workspace(c, mesh_need(k['N']), short, misalign)
    return lib().hnrf_mesh_emit(base.g[tag + 'd'].ptr, k['N'], k['level'], c.put('bmin', k['bmin']), c.put('bmax', k['bmax']), ws, nb,
                                nv, nf, c.new('verts', nv * 12), c.new('faces', nf * 12), _stream())


@functools.lru_cache(maxsize=None)
def mesh_ops(name):
    from humannerf_amd import mesh
    k = ac.mesh_case(name)
    v, f = mesh.mesh_from_density(T(k['d']), k['bmin'], k['bmax'], k['level'])
    torch.cuda.synchronize()
    return v, f


@pytest.mark.parametrize('name', ac.MESH_CASES)
def test_mesh_count_and_emit(name):
    """verts / faces of exactly V / F rows; the level above every density: V = F = 0 and zero-byte buffers."""
    k = ac.mesh_case(name)
    a, b = both(lambda c: run_mesh(c, k))
    same(a, b, ['counts', 'verts', 'faces'])
    v, f = mesh_ops(name)
    assert a.VF == (v.shape[0], f.shape[0]) and (a.VF == (0, 0)) == k['empty']
    eqb(a, 'verts', v), eqb(a, 'faces', f)
    assert a.g['verts'].nbytes == 12 * v.shape[0] and a.g['ws'].nbytes == mesh_need(k['N'])


@pytest.mark.parametrize('name', ['sphere-8', 'open-9'])
def test_mesh_emit_drops_rows_past_v_and_f(name):
    """"Writes past V / F are dropped": with one row fewer of each the guards hold and the kept rows are the same."""
    k = ac.mesh_case(name)
    a, b = both(lambda c: run_mesh(c, k, drop=1))
    same(a, b, ['verts', 'faces'])
    v, f = mesh_ops(name)
    eqb(a, 'verts', v[:-1]), eqb(a, 'faces', f[:-1])


def test_mesh_workspace_reuse_and_refusals():
    k8, k9 = ac.mesh_case('open-8'), ac.mesh_case('sphere-9')
    check_reuse(lambda c: run_mesh(c, k9), lambda c: run_mesh(c, k8), dict(counts=None, verts=None, faces=None), mesh_need(9))
    check_refusals(lambda c, **kw: run_mesh_count(c, k8, **kw), ['counts'])

    def emit_only(c, **kw):                                   # a counted workspace, then the refused emit on another one
        ws, nb = workspace(c, mesh_need(8), **kw)
        return lib().hnrf_mesh_emit(c.put('d', k8['d']), 8, 0.0, c.put('bmin', k8['bmin']), c.put('bmax', k8['bmax']), ws, nb, 5, 5,
                                    c.new('verts', 60), c.new('faces', 60), _stream())
    check_refusals(emit_only, ['verts', 'faces'])


# ========================================================================================== skinning and field normals
SKIN_PARAMS = [(s, e) for s in ac.SKIN_SHAPES for e in ac.SKIN_EXTRA]


@pytest.mark.parametrize('shape,extra', SKIN_PARAMS, ids=str)
def test_forward_skin_and_field_normals(shape, extra):
    """hnrf_forward_skin and hnrf_field_normals: vol of exactly B and of B + 3 channels; vertices on and outside the
    volume's faces, a NaN coordinate; V = 0 launches nothing."""
    from humannerf_amd import ops
    V, B, G = shape
    k = ac.skin_case(V, B, G, extra)

    def skin(c):
        return lib().hnrf_forward_skin(c.put('verts', k['verts']), V, c.put('Rs', k['Rs']), c.put('Ts', k['Ts']), c.put('vol', k['vol']),
                                       B, G, c.put('bmin', k['bmin']), c.put('scale', k['scale']), c.new('out', V * 12), _stream())

    def normals(c):
        return lib().hnrf_field_normals(c.put('verts', k['verts']), c.put('g', k['g']), c.put('sigma', k['sigma']), V,
                                        c.put('vol', k['vol']), B, G, c.put('bmin', k['bmin']), c.put('scale', k['scale']),
                                        c.new('normal', V * 12), _stream())
    a, b = both(skin)
    same(a, b, ['out'])
    dv = {n: T(k[n]) for n in ('verts', 'Rs', 'Ts', 'vol', 'bmin', 'scale', 'g', 'sigma')}
    eqb(a, 'out', ops.forward_skin(dv['verts'], dv['Rs'], dv['Ts'], dv['vol'], dv['bmin'], dv['scale']))
    a, b = both(normals)
    same(a, b, ['normal'])
    eqb(a, 'normal', ops.field_normals(dv['verts'], dv['g'], dv['sigma'], dv['vol'], B, dv['bmin'], dv['scale']))


@pytest.mark.parametrize('K', ac.SKIN_KS)
@pytest.mark.parametrize('shape,extra', SKIN_PARAMS, ids=str)
def test_skin_weights_and_lbs(shape, extra, K):
    """hnrf_skin_weights: joints of exactly V K bytes, kept given and NULL.  hnrf_skin_lbs: mats of exactly B rows and
    joint indices >= B (255 among them): the slot is skipped and nothing past mats is read."""
    from humannerf_amd import ops
    V, B, G = shape
    k = ac.skin_case(V, B, G, extra)
    dv = {n: T(k[n]) for n in ('verts', 'vol', 'bmin', 'scale', 'mats')}
    want = ops.skin_weights(dv['verts'], dv['vol'], B, dv['bmin'], dv['scale'], k=K)
    for with_kept in (True, False):
        def weights(c):
            return lib().hnrf_skin_weights(c.put('verts', k['verts']), V, c.put('vol', k['vol']), B, G, c.put('bmin', k['bmin']),
                                           c.put('scale', k['scale']), K, c.new('joints', V * K), c.new('weights', V * K * 4),
                                           c.new('kept', V * 4) if with_kept else 0, _stream())
        a, b = both(weights)
        outs = ['joints', 'weights'] + (['kept'] if with_kept else [])
        same(a, b, outs)
        for n, t in zip(outs, want):
            eqb(a, n, t)
    j, w = ac.lbs_inputs(k, K)

    def lbs(c):
        return lib().hnrf_skin_lbs(c.put('verts', k['verts']), V, c.put('joints', j), c.put('weights', w), K, c.put('mats', k['mats']), B,
                                   c.new('out', V * 12), _stream())
    a, b = both(lbs)
    same(a, b, ['out'])
    eqb(a, 'out', ops.skin_lbs(dv['verts'], T(j), T(w), dv['mats']))
    assert a.g['joints'].nbytes == V * K and a.g['mats'].nbytes == B * 48


# =========================================================================================================== rasteriser
RASTER_OUTS = [('rgb', 12), ('alpha', 4), ('depth', 4), ('tri_id', 4)]


def run_raster(c, k, H, W, shade, want=('rgb', 'alpha', 'depth', 'tri_id'), short=0, misalign=0):
    from humannerf_amd import raster
    V, F_ = k['verts'].shape[0], k['faces'].shape[0]
    ws, nb = workspace(c, lib().hnrf_raster_workspace_bytes(V, F_, H, W), short, misalign)
    outs = [c.new(n, H * W * sz) if n in want else 0 for n, sz in RASTER_OUTS]
    E = k['E']
    return lib().hnrf_raster_mesh(c.put('verts', k['verts']), V, c.put('faces', k['faces']), F_,
                                  0 if shade == 'normal' else c.put('colors', k['colors']), c.put('K', k['K']),
                                  c.put('R', E[:3, :3]), c.put('T', E[:3, 3]), c.put('bg', k['bg']), H, W, float(F(1e-3)),
                                  raster.CULL['none'] | raster.SHADE[shade], *outs, ws, nb, _stream())


@pytest.mark.parametrize('size', ac.RASTER_SIZES, ids=str)
@pytest.mark.parametrize('scene', ac.RASTER_SCENES)
def test_raster_mesh(scene, size):
    """V = 0, F = 0, face indices outside [0, V), a triangle over the whole image and one hanging over the borders;
    colours NULL with the normal shade; every output given, and each alone with the others NULL; the workspace exact."""
    from humannerf_amd import raster
    H, W = size
    k = ac.raster_case(scene, H, W)
    names = [n for n, _ in RASTER_OUTS]
    for shade in ('color', 'normal'):
        a, b = both(lambda c: run_raster(c, k, H, W, shade))
        same(a, b, names)
        want = raster.rasterize(T(k['verts']), T(k['faces']), None if shade == 'normal' else T(k['colors']), k['K'], k['E'], H, W,
                                bgcolor=k['bg'], shade=shade)
        for n in names:
            eqb(a, n, want[n])
        for n in names if shade == 'color' else names[:1]:
            one, _ = both(lambda c: run_raster(c, k, H, W, shade, want=(n,)))
            assert torch.equal(one.g[n].interior_bytes(), a.g[n].interior_bytes()), n


def test_raster_workspace_reuse_and_refusals():
    big, small = ac.raster_case('cover', 17, 33), ac.raster_case('hang', 5, 7)
    need = lib().hnrf_raster_workspace_bytes(7, 3, 17, 33)
    assert need >= lib().hnrf_raster_workspace_bytes(7, 3, 5, 7) > 0
    check_reuse(lambda c: run_raster(c, big, 17, 33, 'color'), lambda c: run_raster(c, small, 5, 7, 'color'),
                {n: None for n, _ in RASTER_OUTS}, need)
    check_refusals(lambda c, **kw: run_raster(c, small, 5, 7, 'color', **kw), [n for n, _ in RASTER_OUTS])


# ================================================================================================================ LPIPS
@functools.lru_cache(maxsize=None)
def lpips_model():
    from humannerf_amd.lpips import LpipsVGG
    from tests import test_lpips_refs as refs
    return LpipsVGG(refs.trunk(), refs.head_state())


@functools.lru_cache(maxsize=None)
def lpips_packed():
    """The packed image of the ops wrapper, cut to exactly hnrf_lpips_packed_bytes()."""
    p = lpips_model().packed(dev())
    n = lib().hnrf_lpips_packed_bytes()
    torch.cuda.synchronize()
    assert 0 < n <= p.numel() * 4 and n % 256 == 0
    return p.view(torch.uint8)[:n]


@functools.lru_cache(maxsize=None)
def _packed_guarded(fill):
    g = gb.place(lpips_packed(), fill, name='packed', guard=GUARD)
    return g, g.interior_bytes().clone()


def put_packed(c):
    """The packed image in a guarded buffer of exactly its size: one per fill for the whole module (118 MB), its guards
    and its bytes checked by every case that uses it."""
    case = c.case if isinstance(c, Pre) else c
    case.g['packed'], case.orig['packed'] = _packed_guarded(case.fill)
    return case.g['packed'].ptr


def test_lpips_pack():
    """Every weight, bias and head in a buffer of its own; packed of exactly hnrf_lpips_packed_bytes(): every byte of it
    is written (two images of the same weights under the two fills are byte-equal) and equals the wrapper's."""
    m = lpips_model()

    def call(c):
        arr = lambda ts, tag: (ctypes.c_void_p * len(ts))(*[c.put('%s%d' % (tag, i), t) for i, t in enumerate(ts)])
        return lib().hnrf_lpips_pack(arr(m.weights, 'w'), arr(m.biases, 'b'), arr(m.lins, 'lin'),
                                     c.new('packed', lib().hnrf_lpips_packed_bytes()), _stream())
    a, b = both(call)
    same(a, b, ['packed'])
    eqb(a, 'packed', lpips_packed())


def run_conv(c, layer, shape, x, scale, bwd=False, mask=None):
    from humannerf_amd.ops import LPIPS_CONVS
    ci, co = LPIPS_CONVS[layer]
    N, H, W = shape
    if bwd:
        return lib().hnrf_conv3x3_bwd_data(c.put('dy', x), c.put('ys', mask) if mask is not None else 0, put_packed(c), layer, N, H, W,
                                           int(scale), c.new('dx', N * H * W * ci * 4), _stream())
    return lib().hnrf_conv3x3_fwd(c.put('x', x), put_packed(c), layer, N, H, W, int(scale), c.new('y', N * H * W * co * 4), _stream())


def check_conv(layer, shape):
    """x, dy and y_saved in buffers of exactly their size (the first layer's pixels are 3 floats: a float4 load of the
    last one would read 4 bytes past the image); y_saved given and NULL; the layer-0 scaling on and off."""
    from humannerf_amd import ops
    from tests import test_gpu_lpips as tl
    x, dy, ys = tl._conv_inputs(layer, shape, 0)
    pk = lpips_model().packed(dev())
    for scale in ((True, False) if layer == 0 else (False,)):
        a, b = both(lambda c: run_conv(c, layer, shape, x, scale))
        same(a, b, ['y'])
        eqb(a, 'y', ops.conv3x3_fwd(T(x), pk, layer, scale_input=scale))
        for mask in (ys, None):
            a, b = both(lambda c: run_conv(c, layer, shape, dy, scale, bwd=True, mask=mask))
            same(a, b, ['dx'])
            eqb(a, 'dx', ops.conv3x3_bwd_data(T(dy), T(mask), pk, layer, unscale_output=scale))


def _pair_layers():
    from tests import test_gpu_lpips as tl
    return sorted(tl.PAIR_LAYER.values())


@pytest.mark.parametrize('layer', [0, 1, 2, 3, 4, 5, 7, 8])
def test_conv3x3_small_shapes(layer):
    """hnrf_conv3x3_fwd / _bwd_data at the SMALL_SHAPES of tests/test_gpu_lpips.py (1, 4, 30 and 63 pixels) for every
    (Cin, Cout) pair of the trunk."""
    from tests import test_gpu_lpips as tl
    assert layer in _pair_layers() and len(_pair_layers()) == 8
    for shape in tl.SMALL_SHAPES:
        check_conv(layer, shape)


@pytest.mark.parametrize('case', [0, 1, 2])
def test_conv3x3_ragged_last_tile_of_the_large_tilings(case):
    """The three BIG_CASES of tests/test_gpu_lpips.py: the only shapes above 10^4 pixels."""
    from tests import test_gpu_lpips as tl
    layer, shape = tl.BIG_CASES[case]
    check_conv(layer, shape)


@pytest.mark.parametrize('shape', [(2, 3, 5, 64), (1, 7, 9, 128)], ids=str)
def test_maxpool2(shape):
    """Odd sizes drop a row and a column of x; dx is written whole (the dropped row and column with zeros)."""
    from humannerf_amd import ops
    N, H, W, C = shape
    rs = np.random.RandomState(C)
    x = rs.randint(0, 3, shape).astype(F)                                     # exact ties
    dy = rs.standard_normal((N, H // 2, W // 2, C)).astype(F)
    a, b = both(lambda c: lib().hnrf_maxpool2_fwd(c.put('x', x), N, H, W, C, c.new('y', dy.size * 4), _stream()))
    same(a, b, ['y'])
    eqb(a, 'y', ops.maxpool2_fwd(T(x)))
    a, b = both(lambda c: lib().hnrf_maxpool2_bwd(c.put('x', x), c.put('dy', dy), N, H, W, C, c.new('dx', x.size * 4), _stream()))
    same(a, b, ['dx'])
    eqb(a, 'dx', ops.maxpool2_bwd(T(x), T(dy)))


@pytest.mark.parametrize('P', [1, 63])
@pytest.mark.parametrize('C', [64, 512])
def test_lpips_head(C, P):
    """hnrf_lpips_head_fwd: pix_ws of exactly N P floats, layer_val given and NULL, accumulate 0 and 1 (out then holds
    a value before the call: it is an input as well).  hnrf_lpips_head_bwd likewise."""
    from humannerf_amd import ops
    from tests import test_gpu_lpips as tl
    N = 2
    f, w, go = tl._head_inputs(C, P, N)
    prev = np.array([0.25, -1.0], F)
    base = np.random.RandomState(1).standard_normal((N, P, C)).astype(F)
    for acc in (0, 1):
        for with_val in (True, False):
            def fwd(c):
                out = c.put('out', prev) if acc else c.new('out', N * 4)
                c.orig.pop('out', None)                                       # (an accumulator: written on purpose)
                return lib().hnrf_lpips_head_fwd(c.put('f', f), c.put('w', w), N, P, C, c.new('pix', N * P * 4), out, acc,
                                                 c.new('val', N * 4) if with_val else 0, _stream())
            a, b = both(fwd)
            same(a, b, ['out', 'pix'] + (['val'] if with_val else []))
            out, val = ops.lpips_head_fwd(T(f), T(w), out=T(prev) if acc else None, accumulate=bool(acc))
            eqb(a, 'out', out)
            if with_val:
                eqb(a, 'val', val)

        def bwd(c):
            dx = c.put('dx', base) if acc else c.new('dx', N * P * C * 4)
            c.orig.pop('dx', None)
            return lib().hnrf_lpips_head_bwd(c.put('f', f), c.put('w', w), c.put('go', go), N, P, C, dx, acc, _stream())
        a, b = both(bwd)
        same(a, b, ['dx'])
        eqb(a, 'dx', ops.lpips_head_bwd(T(f), T(w), T(go), out=T(base) if acc else None, accumulate=bool(acc)))


LPIPS_SHAPES = [(1, 16, 16, 0), (3, 17, 16, 2)]


def lpips_images(case):
    from tests import test_lpips_refs as refs
    g, key = refs.golden(), refs.case_key(case)
    return tuple(np.ascontiguousarray(g[key + k].transpose(0, 2, 3, 1)) for k in ('_in0', '_in1'))


def lpips_need(case, want_grad):
    return lib().hnrf_lpips_workspace_bytes(case[0], case[1], case[2], want_grad)


def run_lpips_fwd(c, case, want_grad, per=True, short=0, misalign=0, need=None):
    N, H, W, _ = case
    in0, in1 = lpips_images(case)
    ws, nb = workspace(c, lpips_need(case, want_grad) if need is None else need, short, misalign)
    return lib().hnrf_lpips_fwd(c.put('in0', in0), c.put('in1', in1), put_packed(c), N, H, W, want_grad, ws, nb,
                                c.new('out', N * 4), c.new('per', 5 * N * 4) if per else 0, _stream())


def run_lpips_bwd(c, case, short=0, misalign=0):
    N, H, W, _ = case
    go = np.linspace(0.5, 1.5, N).astype(F)
    ws, nb = workspace(c, lpips_need(case, 1), short, misalign)
    return lib().hnrf_lpips_bwd(c.put('go', go), put_packed(c), N, H, W, ws, nb, c.new('d', N * H * W * 12), _stream())


@functools.lru_cache(maxsize=None)
def lpips_ops(case):
    from humannerf_amd import ops
    N, H, W, _ = case
    in0, in1 = (T(a) for a in lpips_images(case))
    pk = lpips_model().packed(dev())
    out, per, ws = ops.lpips_fwd(in0, in1, pk, want_grad=True, want_layers=True)
    d = ops.lpips_bwd(T(np.linspace(0.5, 1.5, N).astype(F)), pk, ws, N, H, W)
    lean = ops.lpips_fwd(in0, in1, pk, want_grad=False, want_layers=True)
    torch.cuda.synchronize()
    assert torch.equal(lean[0], out) and torch.equal(lean[1], per)
    return out, per, d


@pytest.mark.parametrize('case', LPIPS_SHAPES, ids=str)
def test_lpips_fwd_and_bwd(case):
    """want_grad 0 and 1, each in a workspace of its own size; per_layer given and NULL; the backward in the forward's
    workspace."""
    out, per, d = lpips_ops(case)
    assert 0 < lpips_need(case, 0) < lpips_need(case, 1)
    for want_grad in (0, 1):
        a, b = both(lambda c: run_lpips_fwd(c, case, want_grad))
        same(a, b, ['out', 'per'])
        eqb(a, 'out', out), eqb(a, 'per', per)
        assert a.g['ws'].nbytes == lpips_need(case, want_grad)
        a, b = both(lambda c: run_lpips_fwd(c, case, want_grad, per=False))
        same(a, b, ['out'])
        eqb(a, 'out', out)
    a, b = both(lambda c: run_lpips_fwd(c, case, 1) or run_lpips_bwd(c, case))
    same(a, b, ['d', 'out'])
    eqb(a, 'd', d)


def test_lpips_workspace_reuse_and_refusals():
    """hnrf_lpips_bwd after an unrelated shape has run in the same workspace and the forward was repeated; a forward of
    one shape directly after another; the refusals of both entries."""
    small, big = LPIPS_SHAPES
    need = lpips_need(big, 1)
    assert need > lpips_need(small, 1)
    check_reuse(lambda c: run_lpips_fwd(c, big, 1), lambda c: run_lpips_fwd(c, small, 0, need=lpips_need(small, 0)),
                dict(out=None, per=None), need)

    def sequence(c):
        sub = lambda tag: Pre(c, tag)
        return (run_lpips_fwd(sub('first_'), big, 1, need=need) or run_lpips_fwd(sub('other_'), small, 1, need=need)
                or run_lpips_fwd(c, big, 1, need=need) or run_lpips_bwd(c, big))
    a, b = both(sequence)
    same(a, b, ['d', 'out', 'per'])
    eqb(a, 'd', lpips_ops(big)[2]), eqb(a, 'out', lpips_ops(big)[0])
    for want_grad in (0, 1):
        check_refusals(lambda c, **kw: run_lpips_fwd(c, small, want_grad, **kw), ['out', 'per'])
    check_refusals(lambda c, **kw: run_lpips_bwd(c, small, **kw), ['d'])


# ======================================================================================================== image metrics
def run_metrics(c, k, short=0, misalign=0):
    a, b, m = k
    n, H, W = a.shape[:3]
    ws, nb = workspace(c, lib().hnrf_image_metrics_workspace_bytes(n, H, W), short, misalign)
    return lib().hnrf_image_metrics(c.put('pred', a), c.put('target', b), c.put('mask', m) if m is not None else 0, n, H, W, 1.0,
                                    ws, nb, c.new('out', n * 16), _stream())


@pytest.mark.parametrize('mask_kind', ac.METRIC_MASKS)
@pytest.mark.parametrize('size', ac.METRIC_SIZES, ids=str)
@pytest.mark.parametrize('n_img', [1, 3])
def test_image_metrics(n_img, size, mask_kind):
    """out of exactly n_img x 2 doubles; mask NULL, empty, an L whose bounding box exceeds the support, a crop narrower
    than 7 (NaN, no error: the bytes of the NaN are those of the wrapper's)."""
    from humannerf_amd import ops
    k = ac.metrics_case(n_img, size[0], size[1], mask_kind)
    a, b = both(lambda c: run_metrics(c, k))
    same(a, b, ['out'])
    eqb(a, 'out', ops.image_metrics(T(k[0]), T(k[1]), T(k[2])))


def test_image_metrics_workspace_reuse_and_refusals():
    big, small = ac.metrics_case(3, 33, 70, 'L'), ac.metrics_case(1, 8, 9, 'none')
    need = lib().hnrf_image_metrics_workspace_bytes(3, 33, 70)
    assert need >= lib().hnrf_image_metrics_workspace_bytes(1, 8, 9) > 0
    check_reuse(lambda c: run_metrics(c, big), lambda c: run_metrics(c, small), dict(out=None), need)
    check_refusals(lambda c, **kw: run_metrics(c, small, **kw), ['out'])


# =============================================================================================================== clouds
@pytest.mark.parametrize('R', [0, 1, 5])
def test_surface_points(R):
    from humannerf_amd import ops
    for S in (1, 63, 65):
        for B in (1, 24, 32):
            w, xyz, bmw = ac.rays_case(R, S, B)
            a, b = both(lambda c: lib().hnrf_surface_points(c.put('w', w), c.put('xyz', xyz), c.put('bmw', bmw), R, S, B,
                                                             c.new('wxyz', R * 12), c.new('wmax', R * 4), c.new('lbs', R * 4), _stream()))
            same(a, b, ['wxyz', 'wmax', 'lbs'])
            for n, t in zip(('wxyz', 'wmax', 'lbs'), ops.surface_points(T(w), T(xyz), T(bmw))):
                eqb(a, n, t)


@pytest.mark.parametrize('shape', ac.NN_SHAPES, ids=str)
def test_cloud_nn(shape):
    """idx and d2 of exactly Na elements: nothing past Na; Nb = 0 gives -1 / +inf, Na = 0 launches nothing."""
    from humannerf_amd import ops
    Na, Nb = shape
    pa, pb = ac.nn_case(Na, Nb)
    a, b = both(lambda c: lib().hnrf_cloud_nn(c.put('a', pa), Na, c.put('b', pb), Nb, c.new('idx', Na * 4), c.new('d2', Na * 4), _stream()))
    same(a, b, ['idx', 'd2'])
    idx, d2 = ops.cloud_nn(T(pa), T(pb))
    eqb(a, 'idx', idx), eqb(a, 'd2', d2)


def run_pairs(c, k, with_match=True, pairs=None, short=0, misalign=0):
    pairs = k['pairs'] if pairs is None else pairs
    P = len(pairs)
    ws, nb = workspace(c, lib().hnrf_cloud_distance_pairs_workspace_bytes(P, k['max_n']), short, misalign)
    return lib().hnrf_cloud_distance_pairs(c.put('xyz', k['xyz']), c.put('rgb', k['rgb']), c.put('orig', k['orig']),
                                           c.put('offsets', k['offsets']), k['F'], k['total'], c.put('pairs', pairs), P, k['max_n'],
                                           k['axis'], k['tau'], ws, nb, c.new('D', P * 8),
                                           c.new('match', P * k['max_n'] * 4) if with_match else 0, _stream())


def test_cloud_distance_pairs():
    """Frames of 0, 1 and 300 points and one whose offsets row lies outside total; the pairs (i, i), one naming frame 7
    and one naming the frame outside total; match of exactly P max_n, and NULL."""
    from humannerf_amd import ops
    k = ac.pairs_case()
    D, match = ops.cloud_distance_pairs(T(k['xyz']), T(k['rgb']), T(k['orig']), T(k['offsets']), T(k['pairs']), k['tau'], k['axis'],
                                        k['max_n'], want_match=True)
    a, b = both(lambda c: run_pairs(c, k))
    same(a, b, ['D', 'match'])
    eqb(a, 'D', D), eqb(a, 'match', match)
    wantD, want_match = ac.pairs_twin(k)
    assert np.array_equal(match.cpu().numpy(), want_match) and np.array_equal(D.cpu().numpy() > 0, wantD > 0)
    a, b = both(lambda c: run_pairs(c, k, with_match=False))
    same(a, b, ['D'])
    eqb(a, 'D', D)
    more = np.concatenate([k['pairs'][::-1], k['pairs']]).astype(np.int32)    # another shape of the same workspace
    need = lib().hnrf_cloud_distance_pairs_workspace_bytes(8, k['max_n'])
    check_reuse(lambda c: run_pairs(c, k, pairs=more), lambda c: run_pairs(c, k), dict(D=None, match=None), need)
    check_refusals(lambda c, **kw: run_pairs(c, k, **kw), ['D', 'match'])


# ================================================================================================================= JPEG
@pytest.mark.parametrize('q', ac.JPEG_QUALITIES)
@pytest.mark.parametrize('size', ac.JPEG_SIZES, ids=str)
def test_jpeg_header(size, q):
    """hnrf_jpeg_header (host): exactly header_len bytes are written into a host buffer of that many between guards,
    and they are the twin's."""
    from humannerf_amd import video
    H, W = size
    want = video.jpeg_header(H, W, q)
    for fill in (0xFF, 0x00):
        host = (ctypes.c_uint8 * (64 + len(want) + 64))(*([fill] * (128 + len(want))))
        n = lib().hnrf_jpeg_header(H, W, q, ctypes.byref(host, 64), len(want))
        got = bytes(host)
        assert n == len(want) == 613 and got[64:64 + n] == want and got[:64] == got[64 + n:] == bytes([fill]) * 64
        assert lib().hnrf_jpeg_header(H, W, q, ctypes.byref(host, 64), len(want) - 1) == E_ARG and bytes(host) == got


def run_jpeg(c, size, q, pad, short=0, misalign=0):
    from humannerf_amd import video
    H, W = size
    buf, stride = ac.jpeg_tight(ac.jpeg_image(H, W), pad)
    header = np.frombuffer(video.jpeg_header(H, W, q), np.uint8).copy()
    ws, nb = workspace(c, lib().hnrf_jpeg_workspace_bytes(H, W), short, misalign)
    cap = lib().hnrf_jpeg_max_bytes(H, W)
    return lib().hnrf_jpeg_encode(c.put('rgb', buf), H, W, stride, c.put('header', header), header.size, q, ws, nb,
                                  c.new('out', cap), cap, c.new('len', 4), _stream())


@pytest.mark.parametrize('pad', ac.JPEG_PADS)
@pytest.mark.parametrize('q', ac.JPEG_QUALITIES)
@pytest.mark.parametrize('size', ac.JPEG_SIZES, ids=str)
def test_jpeg_encode(size, q, pad):
    """rgb in a TIGHT buffer of (H - 1) row_stride + 3 W bytes (the last row has no padding behind it), header of
    exactly header_len, out of exactly hnrf_jpeg_max_bytes, out_len of 4 bytes.  The bytes of out from *out_len on keep
    the fill; those in front equal the encoder's on the contiguous image and the numpy twin's (the wrapper runs the same
    kernel: an edge pixel replicated from the wrong row or column, which stays inside every buffer and does not depend on
    the fill, shows against the twin alone)."""
    from humannerf_amd import video
    H, W = size
    a, b = both(lambda c: run_jpeg(c, size, q, pad))
    same(a, b, ['len'])
    n = int(a.i('len')[0])
    assert 613 < n <= a.g['out'].nbytes
    same(a, b, ['out'], rows=torch.arange(n), n_rows=n, row_bytes=1)
    for c in (a, b):
        c.g['out'].bytes_hold_fill(n)
    buf, length = video.JpegEncoder(dev(), q).encode(T(ac.jpeg_image(H, W)))
    assert int(length) == n and torch.equal(a.u8('out')[:n], buf[:n])
    assert a.u8('out')[:n].cpu().numpy().tobytes() == video.jpeg_encode_numpy(ac.jpeg_image(H, W), q)    # and the twin's
    assert a.g['rgb'].nbytes == (H - 1) * (3 * W + pad) + 3 * W and a.g['header'].nbytes == 613


def test_jpeg_workspace_reuse_and_refusals():
    big, small = (40, 24), (17, 33)
    need = lib().hnrf_jpeg_workspace_bytes(17, 33)
    assert need >= lib().hnrf_jpeg_workspace_bytes(40, 24) > 0
    n = int(both(lambda c: run_jpeg(c, big, 100, 0))[0].i('len')[0])
    check_reuse(lambda c: run_jpeg(c, small, 100, 21), lambda c: run_jpeg(c, big, 100, 0), {'len': None, 'out': n}, need)
    check_refusals(lambda c, **kw: run_jpeg(c, big, 100, 0, **kw), ['out', 'len'])


# ========================================================================================================= segmentation
def seg_masks(n_parts):
    from humannerf_amd import cloud
    return np.ascontiguousarray(cloud.bone_masks(ac.SEG_PARTS[n_parts]).view(np.int32))


def run_members(c, k, n_parts, radius, short=0, misalign=0):
    masks = seg_masks(n_parts)
    ws, nb = workspace(c, lib().hnrf_segment_workspace_bytes(k['F'], ac.SEG_H, ac.SEG_W), short, misalign)
    return lib().hnrf_segment_members(c.put('rec', k['rec']), c.put('offsets', k['offsets']), k['F'], k['total'], c.put('masks', masks),
                                      masks.size, ac.SEG_H, ac.SEG_W, radius, ws, nb, c.new('member', k['total'] * 4),
                                      c.new('status', 4), _stream())


def compact_need(k, n_parts):
    return lib().hnrf_segment_compact_workspace_bytes(k['total'], n_parts)


def run_count(c, k, member, n_parts, weighted, status=None, short=0, misalign=0):
    ws, nb = workspace(c, compact_need(k, n_parts), short, misalign, name='cws')
    return lib().hnrf_segment_count(c.put('member', member), c.put('wrec', k['rec']) if weighted else 0,
                                    ac.SEG_WEIGHT_MIN if weighted else 0.0, c.put('offsets', k['offsets']), k['F'], k['total'], n_parts,
                                    c.put('status', status) if status is not None else 0, ws, nb,
                                    c.new('seg', (n_parts * k['F'] + 1) * 8), _stream())


def run_scatter(c, k, n_parts, weighted, rows, with_status, short=0, misalign=0):
    """After run_count in the same case: member, wrec, status and the workspace are the count's."""
    base = c.case if isinstance(c, Pre) else c
    tag = c.tag if isinstance(c, Pre) else ''
    ws, nb = workspace(c, compact_need(k, n_parts), short, misalign, name='cws')
    return lib().hnrf_segment_scatter(base.g[tag + 'member'].ptr, base.g[tag + 'wrec'].ptr if weighted else 0,
                                      ac.SEG_WEIGHT_MIN if weighted else 0.0, k['total'], n_parts,
                                      base.g[tag + 'status'].ptr if with_status else 0, ws, nb, c.new('src', rows * 4), rows, _stream())


@pytest.mark.parametrize('n_parts', list(ac.SEG_PARTS))
@pytest.mark.parametrize('radius', ac.SEG_RADII)
def test_segment_members_count_and_scatter(radius, n_parts):
    """Two frames on 7 x 30 pixels, the diamond of radius 33 reaches past every border; two records share a pixel, one
    row lies outside every frame; weight_rec NULL and given (a NaN weight); src of exactly the counted rows, and of one
    row fewer ("not written")."""
    from humannerf_amd import ops
    k = ac.segment_case()
    a, b = both(lambda c: run_members(c, k, n_parts, radius))
    same(a, b, ['member', 'status'])
    member, status = ops.segment_members(T(k['rec']), T(k['offsets']), T(seg_masks(n_parts)), ac.SEG_H, ac.SEG_W, radius)
    eqb(a, 'member', member), eqb(a, 'status', status)
    assert int(status) == 0 and int(member[-1]) == 0
    m = member.cpu().numpy()
    zero = np.zeros(1, np.int32)
    for weighted in (False, True):
        seg, src = ops.segment_compact(member, T(k['offsets']), n_parts, status=status, weight_rec=T(k['rec']) if weighted else None,
                                       weight_min=ac.SEG_WEIGHT_MIN if weighted else 0.0)
        rows = int(seg[-1])
        assert rows == src.numel() > 1
        for drop, with_status in ((0, True), (1, False)):
            a, b = both(lambda c: run_count(c, k, m, n_parts, weighted, zero if with_status else None)
                        or run_scatter(c, k, n_parts, weighted, rows - drop, with_status))
            same(a, b, ['seg', 'src'])
            eqb(a, 'seg', seg), eqb(a, 'src', src[:rows - drop])
            assert a.g['src'].nbytes == 4 * (rows - drop) and a.g['cws'].nbytes == compact_need(k, n_parts)


def test_segment_bad_record_leaves_everything_unwritten():
    """A pixel outside the image raises status bit 2: member, seg_offsets and src hold the fill."""
    k = ac.segment_case(bad=True)
    a, b = both(lambda c: run_members(c, k, 32, 1))
    assert int(a.i('status')[0]) == int(b.i('status')[0]) == 2
    held((a, b), ['member'])
    raised, m = np.array([2], np.int32), np.arange(k['total'], dtype=np.int32)
    a, b = both(lambda c: run_count(c, k, m, 32, True, raised) or run_scatter(c, k, 32, True, 50, True))
    held((a, b), ['seg', 'src', 'cws'])


def test_segment_workspace_reuse_and_refusals():
    k = ac.segment_case()
    from humannerf_amd import ops
    member = ops.segment_members(T(k['rec']), T(k['offsets']), T(seg_masks(32)), ac.SEG_H, ac.SEG_W, 1)[0].cpu().numpy()
    check_reuse(lambda c: run_members(c, k, 1, 33), lambda c: run_members(c, k, 32, 1), dict(member=None, status=None),
                lib().hnrf_segment_workspace_bytes(2, ac.SEG_H, ac.SEG_W))
    check_refusals(lambda c, **kw: run_members(c, k, 32, 1, **kw), ['member', 'status'])
    rows = int(both(lambda c: run_count(c, k, member, 32, False))[0].i64('seg')[-1])
    check_reuse(lambda c: run_count(c, k, member, 32, True) or run_scatter(c, k, 32, True, 7, False),
                lambda c: run_count(c, k, member, 1, False) or run_scatter(c, k, 1, False, 9, False),
                dict(seg=None, src=None), compact_need(k, 32), ws='cws')
    assert rows > 7
    check_refusals(lambda c, **kw: run_count(c, k, member, 32, False, **kw), ['seg'], ws='cws')

    def scatter_only(c, **kw):
        ws, nb = workspace(c, compact_need(k, 32), name='cws', **kw)
        return lib().hnrf_segment_scatter(c.put('member', member), 0, 0.0, k['total'], 32, 0, ws, nb, c.new('src', rows * 4), rows,
                                          _stream())
    check_refusals(scatter_only, ['src'], ws='cws')


# ======================================================================================================== geometry maps
@pytest.mark.parametrize('S', ac.SURFACE_S)
@pytest.mark.parametrize('R', ac.SURFACE_R)
def test_ray_surface(R, S):
    """The full form with every output, each output alone with the others NULL, and the lean form (weights and offsets
    NULL): valid of exactly R bytes."""
    from humannerf_amd import ops
    from tests import geometry_cases as gc
    near, far, alpha, depth, w, off = gc.surface_inputs(R, S, seed=R * 100 + S)
    want = ops.ray_surface(T(near), T(far), T(alpha), T(depth), T(w), T(off), want_median=True, want_woff=True)
    lean = ops.ray_surface(T(near), T(far), T(alpha), T(depth))
    sizes = dict(t_exp=4 * R, t_med=4 * R, woff=12 * R)

    def run(c, outs, full=True):
        ptr = [c.new(n, sizes[n]) if n in outs else 0 for n in ('t_exp', 't_med', 'woff')]
        return lib().hnrf_ray_surface(c.put('near', near), c.put('far', far), c.put('alpha', alpha), c.put('depth', depth),
                                      c.put('w', w) if full else 0, c.put('off', off) if full else 0, R, S, 0.5, *ptr,
                                      c.new('valid', R), _stream())
    for outs in (('t_exp', 't_med', 'woff'), ('t_exp',), ('t_med',), ('woff',), ()):
        a, b = both(lambda c: run(c, outs))
        same(a, b, list(outs) + ['valid'])
        for n in outs:
            eqb(a, n, want[n])
        if 't_med' in outs:
            eqb(a, 'valid', want['valid'])
        else:
            eqb(a, 'valid', want['valid'] & 1)
    a, b = both(lambda c: run(c, ('t_exp',), full=False))
    same(a, b, ['t_exp', 'valid'])
    eqb(a, 't_exp', lean['t_exp']), eqb(a, 'valid', lean['valid'])


MAP_OUTS = dict(normal=12, nvalid=1, normal8=3, depth8=3, shaded8=3, offset8=3)


def run_maps(c, k, H, W, p2r, status, want=tuple(MAP_OUTS), surface=0):
    s = k['surf']
    outs = [c.new(n, H * W * sz) if n in want else 0 for n, sz in MAP_OUTS.items()]
    return lib().hnrf_geometry_maps(c.put('o', k['o']), c.put('d', k['d']), c.put('t_exp', s['t_exp']), c.put('t_med', s['t_med']),
                                    c.put('valid', s['valid']), surface, c.put('alpha', k['alpha']), c.put('woff', s['woff']),
                                    c.put('p2r', p2r), k['N'], H, W, k['edge'], c.put('M', k['M']), c.put('bg', k['bg']),
                                    c.put('lohi', k['lohi']), 0.25, 0.8, c.put('truth', k['truth']),
                                    c.put('status', np.array([status], np.int32)), *outs, _stream())


@pytest.mark.parametrize('size', ac.MAP_SIZES, ids=str)
def test_pixel_rays_and_geometry_maps(size):
    """hnrf_pixel_rays: two rays on one pixel; pix2ray of exactly H W ints.  hnrf_geometry_maps: every panel given, and
    each alone with the others NULL (uint8 panels of 3, 21 and 45 bytes).  A ray index outside the image raises the
    status word, and then pix2ray and every panel hold the fill."""
    from humannerf_amd import ops
    H, W = size
    k = ac.maps_case(H, W)

    def pixel_rays(c, idx):
        return lib().hnrf_pixel_rays(c.put('idx', idx), idx.size, H, W, c.new('p2r', H * W * 4), c.new('status', 4), _stream())
    a, b = both(lambda c: pixel_rays(c, k['ray_index']))
    same(a, b, ['p2r', 'status'])
    dp2r, dst = ops.pixel_rays(T(k['ray_index']), H, W)
    eqb(a, 'p2r', dp2r), eqb(a, 'status', dst)
    assert int(dst) == 0
    p2r = dp2r.cpu().numpy()
    surf = {n: T(v) for n, v in k['surf'].items()}
    for surface in (0, 1):
        want = ops.geometry_maps(T(k['o']), T(k['d']), surf, dp2r, H, W, list(MAP_OUTS), surface=surface, alpha=T(k['alpha']),
                                 edge=k['edge'], M=T(k['M']), bgcolor=T(k['bg']), lohi=T(k['lohi']), truth8=T(k['truth']), status=dst)
        a, b = both(lambda c: run_maps(c, k, H, W, p2r, 0, surface=surface))
        same(a, b, list(MAP_OUTS))
        for n in MAP_OUTS:
            eqb(a, n, want[n])
    for n in MAP_OUTS:
        one, other = both(lambda c: run_maps(c, k, H, W, p2r, 0, want=(n,), surface=1))
        same(one, other, [n])
        eqb(one, n, want[n])
    bad = ac.maps_case(H, W, bad_index=True)
    a, b = both(lambda c: pixel_rays(c, bad['ray_index']))
    assert int(a.i('status')[0]) == int(b.i('status')[0]) == 1
    held((a, b), ['p2r'])
    a, b = both(lambda c: run_maps(c, k, H, W, p2r, 1))
    held((a, b), list(MAP_OUTS))


# ============================================================================================ density-gradient normals
def normals_need(k):
    return lib().hnrf_ray_normals_workspace_bytes(k['R'], k['S'])


def run_ray_normals(c, k, short=0, misalign=0):
    ws, nb = workspace(c, normals_need(k), short, misalign)
    return lib().hnrf_ray_normals(c.put('w', k['w']), c.put('bmw', k['bmw']), c.put('Rs', k['Rs']), c.put('idx', k['idx']),
                                  c.put('count', k['count']), k['n_max'], c.put('g', k['g']), c.put('alpha', k['alpha']), k['R'], k['S'],
                                  k['B'], 0.5, ws, nb, c.new('normal', k['R'] * 12), c.new('nvalid', k['R']), _stream())


@pytest.mark.parametrize('kind', ac.NORMALS_COUNTS)
@pytest.mark.parametrize('shape', ac.NORMALS_SHAPES, ids=str)
def test_ray_normals(shape, kind):
    """idx / g of exactly n_max rows with *count above n_max, equal to it and 0; indices outside [0, R S); nvalid of
    exactly R bytes (1, 3 and 5); the workspace of exactly hnrf_ray_normals_workspace_bytes."""
    from humannerf_amd import ops
    k = ac.ray_normals_case(*shape, kind)
    a, b = both(lambda c: run_ray_normals(c, k))
    same(a, b, ['normal', 'nvalid'])
    n, v = ops.ray_normals(T(k['w']), T(k['bmw']), T(k['Rs']), T(k['idx']), T(k['count']), T(k['g']), T(k['alpha']))
    eqb(a, 'normal', n), eqb(a, 'nvalid', v)
    tn, tv = ac.ray_normals_twin(k)
    assert np.array_equal(v.cpu().numpy(), tv.astype(np.uint8)) and np.array_equal(n.cpu().numpy() == 0, tn == 0)
    assert a.g['nvalid'].nbytes == k['R'] and a.g['ws'].nbytes == normals_need(k) == 4 * k['R'] * k['S']


def test_ray_normals_workspace_reuse_and_refusals():
    """The slot table of another shape in front of the call; a workspace one byte short is HNRF_E_WORKSPACE and one
    misaligned by 4 bytes HNRF_E_ARG, as for every other workspace (include/hnrf.h at hnrf_gen_rays)."""
    big, small = ac.ray_normals_case(5, 65, 24, 'equal'), ac.ray_normals_case(3, 65, 1, 'over')
    check_reuse(lambda c: run_ray_normals(c, big), lambda c: run_ray_normals(c, small), dict(normal=None, nvalid=None),
                normals_need(big))
    check_refusals(lambda c, **kw: run_ray_normals(c, small, **kw), ['normal', 'nvalid'])
    assert 'workspace' in lib().hnrf_last_error().decode()


def test_ray_normals_wrapper_replaces_a_misaligned_workspace():
    """ops.ray_normals given a slice that starts 4 bytes off a 256-byte boundary: it allocates its own."""
    from humannerf_amd import ops
    k = ac.ray_normals_case(3, 65, 24, 'equal')
    args = [T(k[n]) for n in ('w', 'bmw', 'Rs', 'idx', 'count', 'g', 'alpha')]
    want = ops.ray_normals(*args)
    buf = torch.empty(3 * 65 + 64, dtype=torch.int32, device=dev())
    off = (-buf.data_ptr() % 256) // 4 + 1
    got = ops.ray_normals(*args, workspace=buf[off:off + 3 * 65])
    assert buf[off:].data_ptr() % 256 == 4 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize('status', [0, 1])
def test_normal_panels(status):
    """5 x 3 pixels: normal8 / shaded8 of 45 bytes, nvalid of 15; under a raised status word nothing is written."""
    from humannerf_amd import geometry as geo, ops
    from tests import normals_cases as nc
    H, W = 5, 3
    k = nc.panel_case(H, W, seed=15)
    p2r, st = geo.pixel_rays_host(k['ray_index'], H, W)
    assert st == 0
    sizes = dict(normal=12, nvalid=1, normal8=3, shaded8=3)

    def run(c, surface):
        return lib().hnrf_normal_panels(c.put('rays_d', k['rays_d']), c.put('rn', k['normal']), c.put('rv', k['nvalid']),
                                        c.put('valid', k['valid']), surface, c.put('alpha', k['alpha']), c.put('p2r', p2r), k['N'], H, W,
                                        c.put('M', k['M']), c.put('bg', k['bgcolor']), 0.25, 0.8,
                                        c.put('status', np.array([status], np.int32)),
                                        *[c.new(n, H * W * sz) for n, sz in sizes.items()], _stream())
    for surface in (0, 1):
        a, b = both(lambda c: run(c, surface))
        if status:
            held((a, b), list(sizes))
            continue
        same(a, b, list(sizes))
        want = ops.normal_panels(T(k['rays_d']), T(k['normal']), T(k['nvalid']), T(k['valid']), T(p2r), H, W, list(sizes),
                                 surface=surface, alpha=T(k['alpha']), M=T(k['M']), bgcolor=T(k['bgcolor']))
        for n in sizes:
            eqb(a, n, want[n])
