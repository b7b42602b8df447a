"""Host-side operators of the hot path: thin torch-tensor wrappers over the C ABI.

PyTorch is plumbing here (device memory, streams); all arithmetic of the path
happens in libhnrf.so.  Every op requires CUDA(ROCm) fp32 contiguous tensors and
raises otherwise -- there is no eager fallback.
"""
import ctypes

import torch

from . import _lib

MLP_MODES = {'f32': 0, 'f16x3': 1}
# training entry points only: split-f16 arithmetic with the saved weight-gradient operands (activations, dZ) in f16
TRAIN_MODES = {'f32': 0, 'f16x3': 1, 'f16x3h': 2}


NO_RANGE_GUARD, GUARD_ONE_CHUNK = 0x100, 0x200          # hnrf.h: HNRF_MLP_NO_RANGE_GUARD / HNRF_MLP_GUARD_ONE_CHUNK


def _mode_arg(mode):
    """``mode`` argument of the forward entry points: 'f32' | 'f16x3', optionally with the f16-range guard selection
    (hnrf.h) appended -- 'f16x3+noguard' (unguarded kernel instances) or 'f16x3+guard1:<k>' (hnrf_render_frame_fwd:
    only ray chunk k % n_chunks is guarded).  Plain names guard every launch."""
    base, _, opt = mode.partition('+')
    m = MLP_MODES[base]
    if not opt:
        return m
    if opt == 'noguard':
        return m | NO_RANGE_GUARD
    if opt.startswith('guard1:'):
        return m | GUARD_ONE_CHUNK | ((int(opt[7:]) & 0x7fff) << 16)
    raise ValueError('unknown mode option %r' % mode)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise _lib.HnrfError(
                f'hot-path operand must be a contiguous fp32 tensor on the GPU, got '
                f'{t.dtype} {t.device} contiguous={t.is_contiguous()} shape={tuple(t.shape)}')


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def sample_warp(rays_o, rays_d, near, far, t_rand, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale,
                n_samples, want_bmw=False, bmw_out=None):
    """K1 (network.py:455-471, 499, 392-444).  Returns z_vals (R,S), x_skel (R,S,3),
    fg_mask (R,S), bmw (R,S,B) or None.  ``bmw_out``: contiguous (R,S,B) tensor to write bmw into."""
    lib = _lib.load()
    near, far = near.reshape(-1), far.reshape(-1)
    _chk(rays_o, rays_d, near, far, t_rand, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale)
    R, S = rays_o.shape[0], int(n_samples)
    B = motion_Rs.shape[0]
    G = vol.shape[-1]
    assert vol.shape[0] >= B and vol.shape[1] == vol.shape[2] == G
    assert rays_d.shape == (R, 3) and near.numel() == R and far.numel() == R
    if t_rand is not None:
        assert t_rand.shape == (R, S)
    dev = rays_o.device
    z = torch.empty(R, S, device=dev)
    x_skel = torch.empty(R, S, 3, device=dev)
    mask = torch.empty(R, S, device=dev)
    bmw = (bmw_out if bmw_out is not None else torch.empty(R, S, B, device=dev)) if want_bmw else None
    if bmw is not None:
        assert bmw.shape == (R, S, B)
        _chk(bmw)
    _lib.check(lib.hnrf_sample_warp_fwd(_ptr(rays_o), _ptr(rays_d), _ptr(near), _ptr(far), _ptr(t_rand),
                                        _ptr(motion_Rs), _ptr(motion_Ts), _ptr(vol), _ptr(bbox_min),
                                        _ptr(bbox_scale), R, S, B, G, _ptr(z), _ptr(x_skel), _ptr(mask),
                                        _ptr(bmw), _stream()), 'hnrf_sample_warp_fwd')
    return z, x_skel, mask, bmw


def nonrigid_pack(weights, biases, cond, mode='f32', out=None):
    """Pack block_mlps.{0..12} (7 Linear layers) + the frame's condition code."""
    lib = _lib.load()
    m = MLP_MODES[mode]
    cond = cond.reshape(-1)
    _chk(*weights, *biases, cond)
    assert len(weights) == 7 and len(biases) == 7 and cond.numel() == 69
    shapes = [(128, 105), (128, 128), (128, 128), (128, 128), (128, 164), (128, 128), (3, 128)]
    for w, b, s in zip(weights, biases, shapes):
        if tuple(w.shape) != s or b.numel() != s[0]:
            raise _lib.HnrfError(f'non-rigid MLP layer shape {tuple(w.shape)} != {s}: only the default '
                                 f'architecture (default.yaml:142-165) is built')
    nbytes = lib.hnrf_nonrigid_packed_bytes(m)
    if out is None or out.numel() * 4 < nbytes:
        out = torch.empty((nbytes + 3) // 4, device=cond.device)
    _lib.check(lib.hnrf_nonrigid_pack(_ptr_array(weights), _ptr_array(biases), _ptr(cond), m, _ptr(out),
                                      _stream()), 'hnrf_nonrigid_pack')
    return out


def nonrigid(x_skel, hann_w, packed, mode='f32', want_offsets=False, xyz_out=None, offsets_out=None):
    """K2 (hannw_fourier.py:21-49 + mlp_offset.py:74-114).  x_skel (...,3).  ``xyz_out`` / ``offsets_out``:
    contiguous tensors of x_skel's shape to write into."""
    lib = _lib.load()
    _chk(x_skel, hann_w, packed, xyz_out, offsets_out)
    P = x_skel.numel() // 3
    xyz = xyz_out if xyz_out is not None else torch.empty_like(x_skel)
    offsets = (offsets_out if offsets_out is not None else torch.empty_like(x_skel)) if want_offsets else None
    assert xyz.shape == x_skel.shape and (offsets is None or offsets.shape == x_skel.shape)
    _lib.check(lib.hnrf_nonrigid_fwd(_ptr(x_skel), _ptr(hann_w), _ptr(packed), _mode_arg(mode), P, _ptr(xyz),
                                     _ptr(offsets), _stream()), 'hnrf_nonrigid_fwd')
    return xyz, offsets


def _canonical_pack(lib, weights, biases, m, out, n_heads=None):
    """canonical_pack, and with ``n_heads`` canonical_heads_pack: the image of pts_linears.{0..14} (8 layers) +
    output_linear.0, whose rows are the 4 outputs of the one head or of each of the ``n_heads``."""
    _chk(*weights, *biases)
    assert len(weights) == 9 and len(biases) == 9
    shapes = [(256, 63)] + [(256, 256)] * 4 + [(256, 319)] + [(256, 256)] * 2 + [(4 * (n_heads or 1), 256)]
    for w, b, s in zip(weights, biases, shapes):
        if tuple(w.shape) != s or b.numel() != s[0]:
            raise _lib.HnrfError(f'canonical MLP layer shape {tuple(w.shape)} != {s}: only the default architecture '
                                 f'(default.yaml:51-57) {f"with {n_heads} heads of depth 1 " if n_heads else ""}is built')
    nbytes = lib.hnrf_canonical_packed_bytes(m)
    if out is None or out.numel() * 4 < nbytes:
        out = torch.empty((nbytes + 3) // 4, device=weights[0].device)
    ptrs = _ptr_array(weights), _ptr_array(biases)
    if n_heads:
        _lib.check(lib.hnrf_canonical_heads_pack(*ptrs, n_heads, m, _ptr(out), _stream()), 'hnrf_canonical_heads_pack')
    else:
        _lib.check(lib.hnrf_canonical_pack(*ptrs, m, _ptr(out), _stream()), 'hnrf_canonical_pack')
    return out


def canonical_pack(weights, biases, mode='f32', out=None):
    """Pack pts_linears.{0..14} (8 layers) + output_linear.0."""
    return _canonical_pack(_lib.load(), weights, biases, MLP_MODES[mode], out)


def status_word(packed, which, mode):
    """View (1 int32 element, on the device) of a packed image's status word, or None when ``mode`` has none
    (hnrf_canonical_status_offset / hnrf_nonrigid_status_offset): the f16x3 inference kernels OR
    STATUS_F16_RANGE into it when an activation came within reach of the f16 clamp."""
    lib = _lib.load()
    off = (lib.hnrf_canonical_status_offset if which == 'canonical' else lib.hnrf_nonrigid_status_offset)(MLP_MODES[mode.partition('+')[0]])
    if off == 0:
        return None
    assert off % 4 == 0 and packed.dtype == torch.float32
    return packed.view(torch.int32)[off // 4:off // 4 + 1]


STATUS_F16_RANGE = 1


def _mlp_entry(lib, net, stem, n_heads=None):
    """The entry hnrf_<net>_<stem>, or for every head of a multi-head image (``n_heads`` given: 'canonical' only)
    hnrf_canonical_heads_<stem>: (function, name, the n_heads argument that follows P in its list: () or (H,))."""
    name = 'hnrf_%s_%s%s' % (net, '' if n_heads is None else 'heads_', stem)
    return getattr(lib, name), name, () if n_heads is None else (_chk_heads(n_heads),)


def _canonical_fwd(lib, n_heads, xyz, packed, mode, sparse=None, raw=None):
    """K3 (fourier.py:9-38 + mlp_rgb_sigma.py:132-198), and with ``n_heads`` for every head of one trunk pass
    (mlp_rgb_sigma.py:180-193, head_id = -1): xyz (...,3) -> raw (...,4) or (H,...,4).  ``sparse`` = (idx, count): only the
    samples idx[0 .. *count) are written, into ``raw`` or a zeroed tensor."""
    _chk(xyz, packed)
    fn, name, H = _mlp_entry(lib, 'canonical', 'fwd' if sparse is None else 'fwd_sparse', n_heads)
    P = xyz.numel() // 3
    if raw is None:
        raw = (torch.empty if sparse is None else torch.zeros)(*H, *xyz.shape[:-1], 4, device=xyz.device)
    _chk(raw)
    assert raw.numel() == P * 4 * (H[0] if H else 1)
    _lib.check(fn(_ptr(xyz), _ptr(packed), _mode_arg(mode), P, *H, *[_ptr(t) for t in sparse or ()], _ptr(raw), _stream()),
               name)
    return raw


def canonical(xyz, packed, mode='f32'):
    return _canonical_fwd(_lib.load(), None, xyz, packed, mode)


def output_shapes(S, B, diagnostics=True):
    """The keys of a render's output dict (network.py:776-789) with their per-ray trailing shapes for S samples and B
    bones, in the order of autograd.RenderRays.OUTPUT_KEYS: rgb / alpha / depth, and with ``diagnostics`` the other
    eight."""
    shp = {'rgb': (3,), 'alpha': (), 'depth': ()}
    if diagnostics:
        shp.update(weights_on_rays=(S,), rgb_on_rays=(S, 3), cnl_xyz=(3,), cnl_rgb=(3,), cnl_weight=(), xyz_on_rays=(S, 3),
                   backward_motion_weights=(S, B), offsets=(S, 3))
    return shp


def _chk_view_bias(view_bias, R):
    _chk(view_bias)
    if tuple(view_bias.shape) != (R, 3):
        raise _lib.HnrfError(f'view_bias must be ({R}, 3), one colour bias per ray, got {tuple(view_bias.shape)}')


def composite(raw, fg_mask, z_vals, rays_d, xyz, bgcolor, diagnostics=True, cull_eps=0.0, out=None, view_bias=None):
    """K4 (network.py:355-388).  Returns dict with rgb/alpha/depth and, when
    ``diagnostics``, weights_on_rays, rgb_on_rays, cnl_xyz, cnl_rgb, cnl_weight.  ``out``: dict of contiguous
    tensors of those shapes to write into (e.g. row ranges of whole-frame buffers).  ``view_bias`` (R, 3): view-dependent
    colour, added to raw[..., :3] of every sample of the ray in front of the sigmoid (hnrf_composite_view_fwd)."""
    lib = _lib.load() if view_bias is None else _lib.load_view()
    _chk(raw, fg_mask, z_vals, rays_d, xyz, bgcolor)
    R, S = z_vals.shape
    dev = raw.device
    shapes = {k: (R,) + v for k, v in list(output_shapes(S, 0, diagnostics).items())[:8]}    # (K4 writes the first eight)
    if out is None:
        out = {k: torch.empty(*sh, device=dev) for k, sh in shapes.items()}
    else:
        out = {k: out[k] for k in shapes}
        for k, sh in shapes.items():
            assert tuple(out[k].shape) == sh, (k, tuple(out[k].shape), sh)
        _chk(*out.values())
    g = out.get
    if view_bias is not None:
        _chk_view_bias(view_bias, R)
        _lib.check(lib.hnrf_composite_view_fwd(_ptr(raw), _ptr(fg_mask), _ptr(z_vals), _ptr(rays_d), _ptr(xyz),
                                               _ptr(bgcolor), _ptr(view_bias), R, S, float(cull_eps), _ptr(out['rgb']),
                                               _ptr(out['alpha']), _ptr(out['depth']), _ptr(g('weights_on_rays')),
                                               _ptr(g('rgb_on_rays')), _ptr(g('cnl_xyz')), _ptr(g('cnl_rgb')),
                                               _ptr(g('cnl_weight')), _stream()), 'hnrf_composite_view_fwd')
        return out
    _lib.check(lib.hnrf_composite_fwd(_ptr(raw), _ptr(fg_mask), _ptr(z_vals), _ptr(rays_d), _ptr(xyz),
                                      _ptr(bgcolor), R, S, float(cull_eps), _ptr(out['rgb']), _ptr(out['alpha']),
                                      _ptr(out['depth']), _ptr(g('weights_on_rays')), _ptr(g('rgb_on_rays')),
                                      _ptr(g('cnl_xyz')), _ptr(g('cnl_rgb')), _ptr(g('cnl_weight')), _stream()),
               'hnrf_composite_fwd')
    return out


def render_workspace_bytes(R, S):
    return _lib.load().hnrf_render_workspace_bytes(int(R), int(S))


def render_term_workspace_bytes(R, S):
    return _lib.load().hnrf_render_term_workspace_bytes(int(R), int(S))


def _render_args(operands, workspace, need, grow=True):
    """Shared by the render wrappers.  Returns ``operands`` -- their 14 leading tensors, rays_o .. bgcolor -- checked
    and with near / far flattened, and a workspace of at least ``need`` bytes on the rays' device: ``workspace`` itself
    when it is one, else ``need // 4 + 64`` fresh floats (``grow=False``: a caller's workspace that is not one raises)."""
    args = operands[:2] + (operands[2].reshape(-1), operands[3].reshape(-1)) + operands[4:]
    _chk(*args)
    dev = args[0].device
    if workspace is None or workspace.numel() * workspace.element_size() < need or workspace.device != dev:
        if workspace is not None and not grow:
            raise _lib.HnrfError(f'workspace: {workspace.numel() * workspace.element_size()} bytes on '
                                 f'{workspace.device}, need {need} bytes on {dev}')
        workspace = torch.empty(need // 4 + 64, device=dev)
    return args, workspace


def _lean_out(R, dev):
    return {'rgb': torch.empty(R, 3, device=dev), 'alpha': torch.empty(R, device=dev), 'depth': torch.empty(R, device=dev)}


def _render_entry(lib, kind, args, baked, baked_nr, share=False):
    """The hnrf_render_<kind>*_fwd entry that goes with the grids, its name, and the pointers of ``args`` (rays_o ..
    bgcolor) with the grids' arguments in the place of cnl_packed (``baked``) and of hann_w, nr_packed (``baked_nr``).
    ``share`` names hnrf_render_frame_shared_fwd whatever the grids are: render_frame refuses the two together."""
    stem, ptrs, dev = '', list(map(_ptr, args)), args[0].device
    if baked is not None:
        stem, ptrs[12:13] = '_baked', _baked_args(baked, dev)
    if baked_nr is not None:
        stem, ptrs[10:12] = '_baked_nr', _baked_args(baked_nr, dev)
    name = f'hnrf_render_{kind}{"_shared" if share else stem}_fwd'
    return getattr(lib, name), name, ptrs


def render_rays(rays_o, rays_d, near, far, t_rand, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale,
                hann_w, nr_packed, cnl_packed, bgcolor, n_samples, mode='f32', workspace=None, out=None,
                mlp_events=None, cull_eps=0.0, baked=None, baked_nr=None):
    """The whole path for one ray chunk (network.py:474-602) with only the
    rgb/alpha/depth outputs; intermediates live in ``workspace`` (one given must hold
    render_workspace_bytes(R, S) on the rays' device: it is not replaced).  ``mlp_events``:
    optional pair of torch.cuda.Event(enable_timing=True), recorded around the
    canonical-MLP launch.  ``baked``: (grid, bbox_min, bbox_max) of bake_canonical -- raw then comes from the grid
    sampler (hnrf_render_rays_baked_fwd) and ``cnl_packed`` is not used (may be None).  ``baked_nr``: (off_grid, bbox_min,
    bbox_max) of bake_nonrigid, with ``baked`` only -- xyz and raw then come from the fused sampler of the two grids
    (hnrf_render_rays_baked_nr_fwd) and ``hann_w`` / ``nr_packed`` are not used (may be None)."""
    lib = _lib.load()
    _chk_baked_nr(baked, baked_nr)
    R, S = rays_o.shape[0], int(n_samples)
    args, workspace = _render_args((rays_o, rays_d, near, far, t_rand, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale,
                                    hann_w, nr_packed, cnl_packed, bgcolor), workspace,
                                   lib.hnrf_render_workspace_bytes(R, S), grow=False)
    if out is None:
        out = _lean_out(R, rays_o.device)
    ev = (0, 0)
    if mlp_events is not None:
        for e in mlp_events:
            if not e.cuda_event:
                e.record()            # forces creation of the hipEvent_t
        ev = (mlp_events[0].cuda_event, mlp_events[1].cuda_event)
    fn, name, ptrs = _render_entry(lib, 'rays', args, baked, baked_nr)
    _lib.check(fn(*ptrs, _mode_arg(mode), float(cull_eps), R, S, motion_Rs.shape[0],
                  vol.shape[-1], _ptr(workspace), workspace.numel() * workspace.element_size(),
                  _ptr(out['rgb']), _ptr(out['alpha']), _ptr(out['depth']), ev[0], ev[1], _stream()), name)
    return out


_frame_ctx = {}


def _frame_streams(device):
    """Per-device side stream + the 5 events hnrf_render_frame_fwd orders the two streams with."""
    ctx = _frame_ctx.get(device.index)
    if ctx is None:
        side = torch.cuda.Stream(device=device)
        evs = [torch.cuda.Event() for _ in range(5)]
        for e in evs:
            e.record()                       # forces creation of the hipEvent_t
        ctx = _frame_ctx[device.index] = (side, evs)
    return ctx


def _frame_sync_args(dev, N, chunk, overlap, want_mlp_events):
    """What the frame entries order their streams and time their MLP launches with: (side stream or None, its 5 events as
    a C array or None, the 2 x n_chunks MLP events as a C array or None, those events as (start, stop) pairs)."""
    side, ev_arr = None, None
    if overlap and N > chunk:
        side, evs = _frame_streams(dev)
        ev_arr = (ctypes.c_void_p * 5)(*[e.cuda_event for e in evs])
    mlp_arr, pairs = None, []
    if want_mlp_events:
        nchunk = (N + chunk - 1) // chunk
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(nchunk)]
        for a, b in pairs:
            a.record()
            b.record()
        mlp_arr = (ctypes.c_void_p * (2 * nchunk))(*[e.cuda_event for p in pairs for e in p])
    return side, ev_arr, mlp_arr, pairs


def render_frame(rays_o, rays_d, near, far, t_rand, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, hann_w, nr_packed,
                 cnl_packed, bgcolor, n_samples, chunk, mode='f16x3', diagnostics=True, cull_eps=0.0, workspace=None,
                 overlap=True, mlp_event_log=None, baked=None, baked_nr=None, share_log=None, view_bias=None):
    """The whole frame in one call (hnrf_render_frame_fwd): all ray chunks through K1..K4, results in whole-frame tensors;
    K1 of the next chunk on a side stream while the MLP kernels of the current one run.  Returns (dict of outputs,
    workspace).  ``mlp_event_log``: list that receives one (start, stop) torch.cuda.Event pair per chunk.  ``baked``:
    (grid, bbox_min, bbox_max) of bake_canonical -- raw then comes from the grid sampler (hnrf_render_frame_baked_fwd,
    the event pairs around its launches) and ``cnl_packed`` is not used (may be None).  ``baked_nr``: (off_grid, bbox_min,
    bbox_max) of bake_nonrigid, with ``baked`` only -- xyz and raw then come from the fused sampler of the two grids
    (hnrf_render_frame_baked_nr_fwd; xyz_on_rays / offsets are the interpolated values) and ``hann_w`` / ``nr_packed``
    are not used (may be None).  ``share_log``: a list selects hnrf_render_frame_shared_fwd (f16x3, both MLPs, cull_eps == 0;
    the caller has checked that every Hann weight is <= 1) and receives (live_counts, samples): the device int32 tensor
    of the samples per chunk that went through the MLPs, and the frame's sample count.  ``view_bias`` (N, 3): view-dependent
    colour, one raw-colour bias per ray added in K4 -- the frame then goes through hnrf_render_frame_view_fwd, the one entry
    that takes the grids and the shared evaluation as nullable arguments."""
    lib = _lib.load() if view_bias is None else _lib.load_view()
    _chk_baked_nr(baked, baked_nr)
    share = share_log is not None
    if share and (baked is not None or baked_nr is not None):
        raise _lib.HnrfError('render_frame: shared inputs exist with both MLPs only, not with a baked grid')
    out, workspace, live = _frame_call(lib, (rays_o, rays_d, near, far, t_rand, motion_Rs, motion_Ts, vol, bbox_min,
                                             bbox_scale, hann_w, nr_packed, cnl_packed, bgcolor), n_samples, chunk, mode,
                                       diagnostics, cull_eps, workspace, overlap, mlp_event_log, baked, baked_nr, share,
                                       view_bias=view_bias)
    if share:
        share_log.append((live, rays_o.shape[0] * int(n_samples)))
    return out, workspace


HEAD_KEYS = ('rgb', 'alpha', 'depth', 'weights_on_rays', 'rgb_on_rays', 'cnl_xyz', 'cnl_rgb', 'cnl_weight')


def _frame_call(lib, operands, n_samples, chunk, mode, diagnostics, cull_eps, workspace, overlap, mlp_event_log,
                baked=None, baked_nr=None, share=False, n_heads=None, view_bias=None):
    """The one call of a frame entry, for render_frame and -- ``n_heads`` -- render_frame_heads: the workspace, the
    whole-frame output tensors (with ``n_heads`` one allocation per HEAD_KEYS key, head-major: out[k][h] is a contiguous
    whole-frame tensor), the stream and event arguments, the call, and what the side stream and the event log need
    afterwards.  ``share`` with ``n_heads``: hnrf_render_frame_heads_shared_fwd (``lib`` has its header bound).  Returns
    (out, workspace, the live counts of ``share`` or None).  ``view_bias`` (single head): hnrf_render_frame_view_fwd
    (``lib`` has its header bound), the grids, the bias and the live counts as its nullable arguments."""
    H = n_heads
    N, S, B, G = operands[0].shape[0], int(n_samples), operands[5].shape[0], operands[7].shape[-1]
    dev = operands[0].device
    chunk = int(chunk)
    rows = min(chunk, max(N, 1))
    if H:
        stem = 'hnrf_render_frame_heads_shared' if share else 'hnrf_render_frame_heads'
        need = getattr(lib, stem + '_workspace_bytes')(rows, S, H)
    else:
        need = (lib.hnrf_render_frame_shared_workspace_bytes if share else lib.hnrf_render_frame_workspace_bytes)(rows, S)
    args, workspace = _render_args(operands, workspace, need)
    out = {k: torch.empty(((H, N) if H and k in HEAD_KEYS else (N,)) + v, device=dev)
           for k, v in output_shapes(S, B, diagnostics).items()}

    def ptr(k):             # (the heads entry takes the HEAD_KEYS as arrays of one pointer per head)
        if H and k in HEAD_KEYS and k in out:
            return (ctypes.c_void_p * H)(*[out[k][h].data_ptr() for h in range(H)])
        return _ptr(out.get(k))

    side, ev_arr, mlp_arr, pairs = _frame_sync_args(dev, N, chunk, overlap, mlp_event_log is not None)
    if H:
        fn, name, ptrs = getattr(lib, stem + '_fwd'), stem + '_fwd', list(map(_ptr, args))
    elif view_bias is not None:
        _chk_view_bias(view_bias, N)
        no_grid = [None, 0, None, None]
        fn, name, ptrs = lib.hnrf_render_frame_view_fwd, 'hnrf_render_frame_view_fwd', list(map(_ptr, args))
        ptrs[13:13] = (no_grid if baked_nr is None else _baked_args(baked_nr, dev)) + \
            (no_grid if baked is None else _baked_args(baked, dev)) + [_ptr(view_bias)]
    else:
        fn, name, ptrs = _render_entry(lib, 'frame', args, baked, baked_nr, share)
    live = torch.empty(max(1, -(-N // chunk)), dtype=torch.int32, device=dev) if share else None
    _lib.check(fn(
        *ptrs, _mode_arg(mode), float(cull_eps), N, S, B, G, chunk, *([H] if H else []), _ptr(workspace),
        workspace.numel() * workspace.element_size(), *[ptr(k) for k in output_shapes(S, B)],
        *([_ptr(live)] if share or view_bias is not None else []), side.cuda_stream if side is not None else None, ev_arr, mlp_arr, _stream()), name)
    if side is not None:
        # the side stream read the inputs and wrote backward_motion_weights / the workspace: keep the allocator from
        # handing those blocks out again before it is done (everything it did is also ordered on the main stream)
        for t in args[:10] + (workspace, out.get('backward_motion_weights')):      # rays_o .. bbox_scale: K1's inputs
            if t is not None:
                t.record_stream(side)
    if mlp_event_log is not None:
        mlp_event_log.extend(pairs)
    return out, workspace, live


def render_rays_term(rays_o, rays_d, near, far, t_rand, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale,
                     hann_w, nr_packed, cnl_packed, bgcolor, n_samples, mode='f16x3', term_eps=1e-4, cull_eps=0.0,
                     workspace=None, want_count=False):
    """Lean path with early ray termination (opt-in approximation, |d rgb|, |d alpha| <= term_eps): see
    hnrf_render_rays_term_fwd.  Returns the rgb/alpha/depth dict (+ 'evaluated': device int tensor when asked)."""
    lib = _lib.load()
    R, S = rays_o.shape[0], int(n_samples)
    args, workspace = _render_args((rays_o, rays_d, near, far, t_rand, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale,
                                    hann_w, nr_packed, cnl_packed, bgcolor), workspace,
                                   lib.hnrf_render_term_workspace_bytes(R, S))
    out = _lean_out(R, rays_o.device)
    ev = torch.empty(1, dtype=torch.int32, device=rays_o.device) if want_count else None
    _lib.check(lib.hnrf_render_rays_term_fwd(*map(_ptr, args), _mode_arg(mode), float(cull_eps), float(term_eps), R, S,
                                             motion_Rs.shape[0], vol.shape[-1], _ptr(workspace),
                                             workspace.numel() * workspace.element_size(), _ptr(out['rgb']),
                                             _ptr(out['alpha']), _ptr(out['depth']),
                                             None if ev is None else ev.data_ptr(), _stream()),
               'hnrf_render_rays_term_fwd')
    if ev is not None:
        out['evaluated'] = ev
    return out


# ----------------------------------------------------------------------------- training
# The buffers the training kernels save, stated once per network: layers, width, PE columns, sign-mask words per sample
_NET = {'canonical': (8, 256, 63, 8), 'nonrigid': (6, 128, 36, 4)}


def _train_buffers(net, names, P, mode, dev, out=None, lead=()):
    """The buffers ``names`` of a *_train / *_bwd call over P samples:
      pe         (P, PE columns); mode 'f16x3h': row-major float16 (P, 64), the columns behind the PE zero
      acts, dZ   (layers, P, width); 'f16x3h': float16 in the BLOCKED layout of hnrf_mlp_dw_h, (layers, P rounded up to
                 128, width) -- opaque, for mlp_dw_h(..., x_blocked / z_blocked=True)
      bits       (layers, P, words) int32, the relu sign masks
      amax       (layers, 64), max over row l bounds |dZ_l|; 'f16x3h': scale (layers,), the power of two dZ_l was multiplied by
      raw; xyz, offsets; d_xyz, d_x_skel   (*lead, 4); (*lead, 3); (P, 3)
    ``out``: a dict of buffers the caller owns (flat and larger ones will do), taken where it names one -- None = the
    entry's null pointer -- in the place of a fresh tensor."""
    L, W, C, words = _NET[net]
    half = mode == 'f16x3h'
    f = torch.float16 if half else torch.float32
    rows = (P + 127) // 128 * 128 if half else P
    spec = {'pe': ((P, 64 if half else C), f), 'acts': ((L, rows, W), f), 'dZ': ((L, rows, W), f),
            'bits': ((L, P, words), torch.int32), 'amax': ((L,) if half else (L, 64), torch.float32),
            'raw': ((*lead, 4), torch.float32), 'xyz': ((*lead, 3), torch.float32), 'offsets': ((*lead, 3), torch.float32),
            'd_xyz': ((P, 3), torch.float32), 'd_x_skel': ((P, 3), torch.float32)}
    out = out or {}
    return [out[k] if k in out else torch.empty(spec[k][0], dtype=spec[k][1], device=dev) for k in names]


def _mlp_train(lib, net, n_heads, x, hann_w, packed, mode, out, P):
    """canonical_train, nonrigid_train (``hann_w`` given) and canonical_heads_train (``n_heads`` given)."""
    _chk(x, hann_w, packed)
    fn, name, H = _mlp_entry(lib, net, 'fwd_train', n_heads)
    P = x.numel() // 3 if P is None else int(P)
    names = (('raw',) if hann_w is None else ('xyz', 'offsets')) + ('pe', 'acts', 'bits')
    res = _train_buffers(net, names, P, mode, x.device, out, (*H, *x.shape[:-1]))
    _lib.check(fn(_ptr(x), *(() if hann_w is None else (_ptr(hann_w),)), _ptr(packed), TRAIN_MODES[mode], P, *H,
                  *[_ptr(t) for t in res], _stream()), name)
    return tuple(res)


def canonical_train(xyz, packed, mode='f32', *, out=None, P=None):
    """hnrf_canonical_fwd_train: raw (...,4), pe (P,63), acts (8,P,256), relu sign masks (8,P,8) int32 (_train_buffers:
    there also mode 'f16x3h').  ``packed`` must have been made for the same arithmetic (the 'f16x3' image serves
    'f16x3h').  ``out``: buffers of the caller's among raw / pe / acts / bits to write into; ``P``: the sample count
    where xyz is such a larger buffer too."""
    return _mlp_train(_lib.load(), 'canonical', None, xyz, None, packed, mode, out, P)


def canonical_heads_train(xyz, packed, n_heads, mode='f32', *, out=None, P=None):
    """hnrf_canonical_heads_fwd_train: canonical_train on the image of canonical_heads_pack.  raw (H,...,4) head-major;
    pe, acts and the sign masks are canonical_train's (the trunk does not know the heads)."""
    return _mlp_train(_lib.load_heads_train(), 'canonical', n_heads, xyz, None, packed, mode, out, P)


def nonrigid_train(x_skel, hann_w, packed, mode='f32', *, out=None, P=None):
    """hnrf_nonrigid_fwd_train: xyz, offsets, pe (P,36), acts (6,P,128), relu sign masks (6,P,4) int32; mode 'f16x3h':
    float16 acts and a float16 pe (P,64) with columns 36.. zero.  ``out`` / ``P``: as in canonical_train."""
    return _mlp_train(_lib.load(), 'nonrigid', None, x_skel, hann_w, packed, mode, out, P)


def composite_bwd(raw, fg_mask, z_vals, rays_d, bgcolor, g_rgb, g_alpha=None, g_depth=None, d_raw_out=None,
                  view_bias=None):
    """K4'.  ``d_raw_out``: a contiguous tensor of raw's size to write d_raw into (one plane of a multi-head d_raw).
    ``view_bias`` (R, 3): the forward's view-dependent colour bias; then (d_raw, d_mask, d_bias (R, 3)) is returned
    (hnrf_composite_view_bwd)."""
    lib = _lib.load() if view_bias is None else _lib.load_view()
    _chk(raw, fg_mask, z_vals, rays_d, bgcolor, g_rgb, g_alpha, g_depth, d_raw_out)
    R, S = z_vals.shape
    assert d_raw_out is None or d_raw_out.numel() == raw.numel()
    d_raw, d_mask = torch.empty_like(raw) if d_raw_out is None else d_raw_out, torch.empty_like(fg_mask)
    if view_bias is not None:
        _chk_view_bias(view_bias, R)
        d_bias = torch.empty_like(view_bias)
        _lib.check(lib.hnrf_composite_view_bwd(_ptr(raw), _ptr(fg_mask), _ptr(z_vals), _ptr(rays_d), _ptr(bgcolor),
                                               _ptr(view_bias), _ptr(g_rgb), _ptr(g_alpha), _ptr(g_depth), R, S, _ptr(d_raw),
                                               _ptr(d_mask), _ptr(d_bias), _stream()), 'hnrf_composite_view_bwd')
        return d_raw, d_mask, d_bias
    _lib.check(lib.hnrf_composite_bwd(_ptr(raw), _ptr(fg_mask), _ptr(z_vals), _ptr(rays_d), _ptr(bgcolor), _ptr(g_rgb),
                                      _ptr(g_alpha), _ptr(g_depth), R, S, _ptr(d_raw), _ptr(d_mask), _stream()),
               'hnrf_composite_bwd')
    return d_raw, d_mask


def view_bias(dirs, B, c):
    """The per-ray colour bias of view-dependent colour (hnrf_view_bias_fwd): dirs (R, 3) of any length, B (3, 3 + 6 L),
    c (3,) -> B e(d) + c (R, 3), e the reference's direction embedding of normalize(d)."""
    lib = _lib.load_view()
    c = c.reshape(-1)
    _chk(dirs, B, c)
    R, L = dirs.shape[0], (B.shape[1] - 3) // 6
    if dirs.shape != (R, 3) or tuple(B.shape) != (3, 3 + 6 * L) or c.numel() != 3:
        raise _lib.HnrfError(f'view_bias: dirs (R, 3), B (3, 3 + 6 L), c (3,), got {tuple(dirs.shape)}, {tuple(B.shape)}, '
                             f'{tuple(c.shape)}')
    out = torch.empty(R, 3, device=dirs.device)
    _lib.check(lib.hnrf_view_bias_fwd(_ptr(dirs), _ptr(B), _ptr(c), L, R, _ptr(out), _stream()), 'hnrf_view_bias_fwd')
    return out


def view_bias_bwd(dirs, d_bias, L):
    """Backward of view_bias with respect to B and c (hnrf_view_bias_bwd, a fixed-order two-stage sum): (dB (3, 3 + 6 L),
    dc (3,))."""
    lib = _lib.load_view()
    _chk(dirs, d_bias)
    R, L = dirs.shape[0], int(L)
    assert dirs.shape == (R, 3) and d_bias.shape == (R, 3)
    need = lib.hnrf_view_bias_bwd_workspace_bytes(R, L)
    if need == 0:
        raise _lib.HnrfError(f'view_bias_bwd: L={L} outside 1..10')
    ws = torch.empty(need // 4 + 64, device=dirs.device)
    dB, dc = torch.empty(3, 3 + 6 * L, device=dirs.device), torch.empty(3, device=dirs.device)
    _lib.check(lib.hnrf_view_bias_bwd(_ptr(dirs), _ptr(d_bias), L, R, _ptr(ws), ws.numel() * 4, _ptr(dB), _ptr(dc),
                                      _stream()), 'hnrf_view_bias_bwd')
    return dB, dc


def pe_bwd(x, g, hann_w, n_bands, include_input, out=None):
    """d PE -> d position; accumulates into ``out`` when given."""
    lib = _lib.load()
    _chk(x, g, hann_w, out)
    P = x.numel() // 3
    assert g.shape[-1] == (3 if include_input else 0) + 6 * n_bands and g.numel() // g.shape[-1] == P
    acc = out is not None
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.hnrf_pe_bwd(_ptr(x), _ptr(g), _ptr(hann_w), P, n_bands, int(include_input), int(acc), _ptr(out),
                               _stream()), 'hnrf_pe_bwd')
    return out


def _mlp_bwd_pack(lib, net, n_heads, weights, mode, out):
    _chk(*weights)
    fn, name, H = _mlp_entry(lib, net, 'bwd_pack', n_heads)
    assert len(weights) == _NET[net][0] + 1 and (not H or tuple(weights[8].shape) == (4 * H[0], 256))
    m = MLP_MODES[mode]
    nbytes = _mlp_entry(lib, net, 'bwd_packed_bytes', n_heads)[0](m, *H)
    if out is None or out.numel() * 4 < nbytes:
        out = torch.empty((nbytes + 3) // 4, device=weights[0].device)
    _lib.check(fn(_ptr_array(weights), *H, m, _ptr(out), _stream()), name)
    return out


def canonical_bwd_pack(weights, mode='f32', out=None):
    """hnrf_canonical_bwd_pack: the transposed image of the 9 canonical nn.Linear weights the dX chain reads, for a
    caller that keeps it (canonical_bwd packs one per call).  ``out``: a buffer of a former pack to write into."""
    return _mlp_bwd_pack(_lib.load(), 'canonical', None, weights, mode, out)


def canonical_heads_bwd_pack(weights, n_heads, mode='f32', out=None):
    """hnrf_canonical_heads_bwd_pack: as canonical_bwd_pack, with weights[8] (4 H, 256)."""
    return _mlp_bwd_pack(_lib.load_heads_train(), 'canonical', n_heads, weights, mode, out)


def nonrigid_bwd_pack(weights, mode='f32', out=None):
    """hnrf_nonrigid_bwd_pack: as canonical_bwd_pack, of the 7 non-rigid nn.Linear weights."""
    return _mlp_bwd_pack(_lib.load(), 'nonrigid', None, weights, mode, out)


def _mlp_bwd(lib, net, n_heads, x, hann_w, d_in, bits, weights, mode, out, bound, P):
    """canonical_bwd, nonrigid_bwd (``hann_w`` given) and canonical_heads_bwd (``n_heads`` given): -> dZ, d_x, amax."""
    _chk(x, hann_w, d_in, bound)
    fn, name, H = _mlp_entry(lib, net, 'bwd', n_heads)
    exact = P is None                   # else the operands may be larger buffers of which P samples count
    P = x.numel() // 3 if exact else int(P)
    L, _, _, words = _NET[net]
    n_bits, n_in = L * P * words, (3 if hann_w is not None else 4 * (H[0] if H else 1)) * P
    assert bits.dtype == torch.int32 and bits.is_contiguous()
    assert (bits.shape == (L, P, words) and d_in.numel() == n_in) if exact else (bits.numel() >= n_bits and d_in.numel() >= n_in)
    if torch.is_tensor(weights):
        packed = weights
        _chk(packed)
    else:
        packed = _mlp_bwd_pack(lib, net, n_heads, weights, 'f16x3' if mode == 'f16x3h' else mode, None)
    if bound is None and mode != 'f32':
        bound = d_in.abs().amax().reshape(1)
    dZ, d_x, amax = _train_buffers(net, ('dZ', 'd_xyz' if hann_w is None else 'd_x_skel', 'amax'), P, mode, x.device, out)
    _lib.check(fn(_ptr(x), *(() if hann_w is None else (_ptr(hann_w),)), _ptr(d_in), _ptr(bits), _ptr(packed),
                  TRAIN_MODES[mode], _ptr(bound), P, *H, _ptr(dZ), _ptr(d_x), _ptr(amax), _stream()), name)
    return dZ, d_x, amax


def canonical_bwd(xyz, d_raw, bits, weights, mode='f32', *, out=None, d_raw_amax=None, P=None):
    """dX chain of the canonical MLP: returns dZ (8,P,256), d_xyz (P,3) and amax (8,64) (max over row l bounds
    |dZ_l|).  bits: sign masks from canonical_train.  mode 'f16x3h': dZ is float16 in the chain's scaled domain and the
    third result is scale (8,): the power of two dZ_l was multiplied by (mlp_dw_h divides it out).  ``weights``: the 9
    nn.Linear weights, packed here, or the backward image (canonical_bwd_pack: one tensor).  ``out``: buffers of the
    caller's among dZ / d_xyz / amax (_train_buffers); ``d_raw_amax``: a device scalar >= max |d_raw|, taken here
    otherwise; ``P``: the sample count where the operands are larger buffers."""
    return _mlp_bwd(_lib.load(), 'canonical', None, xyz, None, d_raw, bits, weights, mode, out, d_raw_amax, P)


def canonical_heads_bwd(xyz, d_raw, bits, weights, n_heads, mode='f32', *, out=None, d_raw_amax=None, P=None):
    """canonical_bwd seeded with every head's gradient: d_raw (H,P,4) head-major, weights[8] (4 H, 256) or the image of
    canonical_heads_bwd_pack.  Returns what canonical_bwd returns; the bound of the incoming gradient is taken over all
    planes."""
    return _mlp_bwd(_lib.load_heads_train(), 'canonical', n_heads, xyz, None, d_raw, bits, weights, mode, out, d_raw_amax, P)


def nonrigid_bwd(x_skel, hann_w, d_xyz, bits, weights, mode='f32', *, out=None, d_xyz_amax=None, P=None):
    """dX chain of the non-rigid MLP: returns dZ (6,P,128), d_x_skel (P,3) (identity path included), amax (6,64)
    (mode 'f16x3h': float16 dZ and scale (6,)); the keyword arguments as in canonical_bwd."""
    return _mlp_bwd(_lib.load(), 'nonrigid', None, x_skel, hann_w, d_xyz, bits, weights, mode, out, d_xyz_amax, P)


_dw_ws = {}


def _dw_workspace(need, device):
    """The device's weight-gradient workspace of at least ``need`` bytes: kept between calls, grown when too small."""
    ws = _dw_ws.get(device.index)
    if ws is None or ws.numel() < need:
        ws = _dw_ws[device.index] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def _db_buffer(db_out, n_out, want_db, device):
    if db_out is None:
        return torch.empty(n_out, device=device) if want_db else None
    assert db_out.dtype == torch.float32 and db_out.is_cuda and db_out.is_contiguous() and db_out.numel() == n_out
    return db_out


def mlp_dw(dZ, X, dW_out=None, want_db=True, mode='f32', dz_amax=None, db_out=None):
    """dW = dZ^T X (and db = column sums of dZ) for one nn.Linear: dZ [P, n_out], X [P, n_in], row-major views
    whose last dimension is contiguous.  ``dW_out``: optional [n_out, >= n_in] view to write into (row stride kept).
    mode 'f16x3' (matrix-shaped layers only, others fall back to fp32 MFMA) needs ``dz_amax``: a device scalar
    tensor whose maximum bounds |dZ| (one row of the chain kernels' amax output).  ``db_out``: optional contiguous
    [n_out] view for db (the rows of one head in a multi-head gradient)."""
    lib = _lib.load()
    assert dZ.dtype == torch.float32 and X.dtype == torch.float32 and dZ.is_cuda and X.is_cuda
    assert dZ.dim() == 2 and X.dim() == 2 and dZ.stride(1) == 1 and X.stride(1) == 1 and dZ.shape[0] == X.shape[0]
    P, n_out = dZ.shape
    n_in = X.shape[1]
    if dW_out is None:
        dW_out = torch.empty(n_out, n_in, device=dZ.device)
    assert dW_out.stride(1) == 1 and dW_out.shape[0] == n_out and dW_out.shape[1] == n_in
    db = _db_buffer(db_out, n_out, want_db, dZ.device)
    need = lib.hnrf_mlp_dw_workspace_bytes(P, n_out, n_in)
    if need == 0:
        raise _lib.HnrfError('hnrf_mlp_dw: shape (%d, %d, %d) not built' % (P, n_out, n_in))
    ws = _dw_workspace(need, dZ.device)
    if mode == 'f16x3' and dz_amax is None:
        dz_amax = dZ.abs().amax().reshape(1)
    _lib.check(lib.hnrf_mlp_dw(dZ.data_ptr(), dZ.stride(0), X.data_ptr(), X.stride(0), P, n_out, n_in,
                               MLP_MODES[mode], _ptr(dz_amax), 0 if dz_amax is None else dz_amax.numel(),
                               dW_out.data_ptr(), dW_out.stride(0), _ptr(db), ws.data_ptr(), ws.numel(), _stream()),
               'hnrf_mlp_dw')
    return dW_out, db


def mlp_dw_h(dZ, X, dW_out=None, want_db=True, dz_scale=None, n_in=None, P=None, z_blocked=False, x_blocked=False,
             db_out=None):
    """hnrf_mlp_dw_h: dW = dZ^T X / scale (and db) from f16 operands.  dZ [P, n_out] f16 (n_out 128 | 256) or, for a
    head, fp32 [P, n_out <= 4]; X [P, >= n_in] f16 whose rows are zero-padded to 64 / 128 / 256 columns; ``n_in``:
    columns of dW (default X.shape[1]); dz_scale: device scalar the stored dZ was multiplied by.  ``z_blocked`` /
    ``x_blocked``: the matrix is one layer of the blocked buffers canonical_train / canonical_bwd return in mode
    'f16x3h' (shape [P padded to 128, width]); ``P`` then gives the true sample count."""
    lib = _lib.load()
    head = dZ.shape[1] <= 4
    assert X.dtype == torch.float16 and dZ.dtype == (torch.float32 if head else torch.float16) and dZ.is_cuda and X.is_cuda
    assert dZ.dim() == 2 and X.dim() == 2 and dZ.stride(1) == 1 and X.stride(1) == 1
    n_out = dZ.shape[1]
    P = int(dZ.shape[0] if P is None else P)
    assert dZ.shape[0] >= P and X.shape[0] >= P and (z_blocked or x_blocked or dZ.shape[0] == X.shape[0])
    assert (not z_blocked or dZ.is_contiguous()) and (not x_blocked or X.is_contiguous())
    n_in = int(X.shape[1] if n_in is None else n_in)
    if dW_out is None:
        dW_out = torch.empty(n_out, n_in, device=dZ.device)
    assert dW_out.stride(1) == 1 and dW_out.shape[0] == n_out and dW_out.shape[1] == n_in and dW_out.dtype == torch.float32
    db = _db_buffer(db_out, n_out, want_db, dZ.device)
    need = lib.hnrf_mlp_dw_h_workspace_bytes(P, n_out, n_in)
    if need == 0:
        raise _lib.HnrfError('hnrf_mlp_dw_h: shape (%d, %d, %d) not built' % (P, n_out, n_in))
    ws = _dw_workspace(need, dZ.device)
    layout = (1 if z_blocked else 0) | (2 if x_blocked else 0)
    _lib.check(lib.hnrf_mlp_dw_h(dZ.data_ptr(), dZ.stride(0), X.data_ptr(), X.stride(0), P, n_out, n_in, layout,
                                 _ptr(dz_scale), dW_out.data_ptr(), dW_out.stride(0), _ptr(db), ws.data_ptr(), ws.numel(),
                                 _stream()), 'hnrf_mlp_dw_h')
    return dW_out, db


def motion_basis_fwd(dst_Rs, dst_Ts, cnl_gtfms, want_saved=False, rvec=None):
    """hnrf_motion_basis_fwd: (B,3,3), (B,3), (B,4,4) -> Rs (B,3,3), Ts (B,3) [, saved state for the backward].
    With ``rvec`` (B-1,3): hnrf_refined_motion_basis_fwd (the pose refinement's Rodrigues correction folded in)."""
    lib = _lib.load()
    _chk(dst_Rs, dst_Ts, cnl_gtfms)
    B = dst_Rs.shape[0]
    assert dst_Rs.shape == (B, 3, 3) and dst_Ts.shape == (B, 3) and cnl_gtfms.shape == (B, 4, 4)
    Rs, Ts = torch.empty_like(dst_Rs), torch.empty_like(dst_Ts)
    saved = torch.empty(lib.hnrf_motion_basis_saved_bytes() // 8, dtype=torch.float64, device=dst_Rs.device) if want_saved else None
    if rvec is None:
        _lib.check(lib.hnrf_motion_basis_fwd(_ptr(dst_Rs), _ptr(dst_Ts), _ptr(cnl_gtfms), B, _ptr(Rs), _ptr(Ts), _ptr(saved),
                                             _stream()), 'hnrf_motion_basis_fwd')
    else:
        _chk(rvec)
        assert rvec.shape == (B - 1, 3)
        _lib.check(lib.hnrf_refined_motion_basis_fwd(_ptr(rvec), _ptr(dst_Rs), _ptr(dst_Ts), _ptr(cnl_gtfms), B, _ptr(Rs),
                                                     _ptr(Ts), _ptr(saved), _stream()), 'hnrf_refined_motion_basis_fwd')
    return Rs, Ts, saved


def motion_basis_bwd(g_Rs, g_Ts, dst_Rs, dst_Ts, cnl_gtfms, saved, rvec=None):
    """-> d_dst_Rs, d_dst_Ts [, d_rvec when ``rvec`` is given]."""
    lib = _lib.load()
    _chk(g_Rs, g_Ts, dst_Rs, dst_Ts, cnl_gtfms)
    d_Rs, d_Ts = torch.empty_like(dst_Rs), torch.empty_like(dst_Ts)
    if rvec is None:
        _lib.check(lib.hnrf_motion_basis_bwd(_ptr(g_Rs), _ptr(g_Ts), _ptr(dst_Rs), _ptr(dst_Ts), _ptr(cnl_gtfms), dst_Rs.shape[0],
                                             _ptr(saved), _ptr(d_Rs), _ptr(d_Ts), _stream()), 'hnrf_motion_basis_bwd')
        return d_Rs, d_Ts
    _chk(rvec)
    d_rvec = torch.empty_like(rvec)
    _lib.check(lib.hnrf_refined_motion_basis_bwd(_ptr(g_Rs), _ptr(g_Ts), _ptr(rvec), _ptr(dst_Rs), _ptr(dst_Ts), _ptr(cnl_gtfms),
                                                 dst_Rs.shape[0], _ptr(saved), _ptr(d_rvec), _ptr(d_Rs), _ptr(d_Ts), _stream()),
               'hnrf_refined_motion_basis_bwd')
    return d_Rs, d_Ts, d_rvec


def _pose_mlp_dims(weights):
    import ctypes
    dims = [int(weights[0].shape[1])] + [int(w.shape[0]) for w in weights]
    for l, w in enumerate(weights):
        assert tuple(w.shape) == (dims[l + 1], dims[l]), 'layer %d: %s' % (l, tuple(w.shape))
    return (ctypes.c_int * len(dims))(*dims), dims


def pose_mlp_fwd(x, weights, biases):
    """hnrf_pose_mlp_fwd: x (n_in,) through Linear+ReLU ... Linear -> (n_out,), saved state for the backward."""
    lib = _lib.load()
    _chk(x, *weights, *biases)
    cdims, dims = _pose_mlp_dims(weights)
    L = len(weights)
    out = torch.empty(dims[-1], device=x.device)
    saved = torch.empty(lib.hnrf_pose_mlp_saved_bytes(L) // 4, device=x.device)
    _lib.check(lib.hnrf_pose_mlp_fwd(_ptr(x), _ptr_array(weights), _ptr_array(biases), cdims, L, _ptr(out), _ptr(saved),
                                     _stream()), 'hnrf_pose_mlp_fwd')
    return out, saved


def pose_mlp_bwd(g_out, x, weights, biases, saved, want_dx=False):
    """-> [dW_l], [db_l], d_x or None."""
    lib = _lib.load()
    _chk(g_out, x, saved, *weights, *biases)
    cdims, dims = _pose_mlp_dims(weights)
    dW = [torch.empty_like(w) for w in weights]
    db = [torch.empty_like(b) for b in biases]
    parts = torch.empty(8, 256, device=x.device) if want_dx else None
    _lib.check(lib.hnrf_pose_mlp_bwd(_ptr(g_out), _ptr(x), _ptr_array(weights), _ptr_array(biases), cdims, len(weights),
                                     _ptr(saved), _ptr_array(dW), _ptr_array(db), _ptr(parts), _stream()), 'hnrf_pose_mlp_bwd')
    d_x = parts[:(dims[1] + 31) // 32, :dims[0]].sum(0) if want_dx else None
    return dW, db, d_x


def sample_warp_bwd(rays_o, rays_d, z_vals, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, x_skel, fg_mask,
                    g_x_skel, g_mask):
    """Returns d_vol (same shape as vol; background channel zero), d_Rs (B,3,3), d_Ts (B,3)."""
    lib = _lib.load()
    _chk(rays_o, rays_d, z_vals, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, x_skel, fg_mask, g_x_skel, g_mask)
    R, S = z_vals.shape
    B, G = motion_Rs.shape[0], vol.shape[-1]
    d_vol = torch.zeros_like(vol)
    d_Rs, d_Ts = torch.empty_like(motion_Rs), torch.empty_like(motion_Ts)
    _lib.check(lib.hnrf_sample_warp_bwd(_ptr(rays_o), _ptr(rays_d), _ptr(z_vals), _ptr(motion_Rs), _ptr(motion_Ts),
                                        _ptr(vol), _ptr(bbox_min), _ptr(bbox_scale), _ptr(x_skel), _ptr(fg_mask),
                                        _ptr(g_x_skel), _ptr(g_mask), R, S, B, G, _ptr(d_vol), _ptr(d_Rs), _ptr(d_Ts),
                                        _stream()), 'hnrf_sample_warp_bwd')
    return d_vol, d_Rs, d_Ts


# ----------------------------------------------------------------------------- sample culling
def compact_samples(fg_mask, eps):
    """idx (P,) int32 and count (1,) int32 (device): samples with fg_mask >= eps."""
    lib = _lib.load()
    _chk(fg_mask)
    P = fg_mask.numel()
    idx = torch.empty(P, dtype=torch.int32, device=fg_mask.device)
    count = torch.empty(1, dtype=torch.int32, device=fg_mask.device)
    _lib.check(lib.hnrf_compact_samples(_ptr(fg_mask), float(eps), P, _ptr(idx), _ptr(count), _stream()),
               'hnrf_compact_samples')
    return idx, count


def canonical_sparse(xyz, packed, idx, count, mode='f32', raw=None):
    return _canonical_fwd(_lib.load(), None, xyz, packed, mode, (idx, count), raw)


# ----------------------------------------------------------------------------- multi-head canonical MLP
HEADS_MIN, HEADS_MAX = 2, 8          # the head layer is one 32-row MFMA tile: up to 8 heads x 4 outputs


def _chk_heads(n_heads):
    n_heads = int(n_heads)
    if not HEADS_MIN <= n_heads <= HEADS_MAX:
        raise _lib.HnrfError(f'n_heads = {n_heads}: the multi-head canonical MLP is built for {HEADS_MIN}..{HEADS_MAX} heads')
    return n_heads


def canonical_heads_pack(weights, biases, n_heads, mode='f32', out=None):
    """canonical_pack for the multi-head MLP (mlp_rgb_sigma.py:114-115): output_linear.0 is (4 n_heads, 256).  The image
    is for canonical_heads / render_frame_heads only; a single head is packed by canonical_pack from its four rows."""
    lib = _lib.load_heads()
    m, H = MLP_MODES[mode], _chk_heads(n_heads)
    return _canonical_pack(lib, weights, biases, m, out, H)


def canonical_heads(xyz, packed, n_heads, mode='f32'):
    return _canonical_fwd(_lib.load_heads(), n_heads, xyz, packed, mode)


def canonical_heads_sparse(xyz, packed, n_heads, idx, count, mode='f32', raw=None):
    return _canonical_fwd(_lib.load_heads(), n_heads, xyz, packed, mode, (idx, count), raw)


def render_frame_heads(rays_o, rays_d, near, far, t_rand, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale, hann_w,
                       nr_packed, cnl_packed, bgcolor, n_samples, chunk, n_heads, mode='f16x3', diagnostics=True,
                       cull_eps=0.0, workspace=None, overlap=True, mlp_event_log=None, share_log=None):
    """render_frame for every head of a multi-head image (hnrf_render_frame_heads_fwd; network.py:570-601): the MLP
    trunks once per chunk, one compositing pass per head.  Returns (dict, workspace): the HEAD_KEYS are lists of n_heads
    whole-frame tensors, xyz_on_rays is the same tensor n_heads times, backward_motion_weights and offsets are tensors.
    ``share_log``: as in render_frame -- a list selects hnrf_render_frame_heads_shared_fwd and receives (live_counts,
    samples); a live sample counts once, not once per head."""
    share = share_log is not None
    lib = _lib.load_heads_shared() if share else _lib.load_heads()
    H = _chk_heads(n_heads)
    out, workspace, live = _frame_call(lib, (rays_o, rays_d, near, far, t_rand, motion_Rs, motion_Ts, vol, bbox_min,
                                             bbox_scale, hann_w, nr_packed, cnl_packed, bgcolor), n_samples, chunk, mode,
                                       diagnostics, cull_eps, workspace, overlap, mlp_event_log, share=share, n_heads=H)
    if share:
        share_log.append((live, rays_o.shape[0] * int(n_samples)))
    out = {k: list(v.unbind(0)) if k in HEAD_KEYS else v for k, v in out.items()}
    if 'xyz_on_rays' in out:
        out['xyz_on_rays'] = [out['xyz_on_rays']] * H
    return out, workspace


def nonrigid_sparse(x_skel, hann_w, packed, idx, count, mode='f32'):
    lib = _lib.load()
    _chk(x_skel, hann_w, packed)
    P = x_skel.numel() // 3
    xyz = x_skel.clone()
    _lib.check(lib.hnrf_nonrigid_fwd_sparse(_ptr(x_skel), _ptr(hann_w), _ptr(packed), _mode_arg(mode), P, _ptr(idx),
                                            _ptr(count), _ptr(xyz), 0, _stream()), 'hnrf_nonrigid_fwd_sparse')
    return xyz


def gen_rays(K, E, bbox_min, bbox_max, H, W, device=None, camera_turn=None):
    """Rays of one camera that cross the bbox, generated on the device in pixel order.

    K (3,3), E (4,4) float32 arrays / tensors (intrinsics, world->camera extrinsics), bbox_min / bbox_max (3,).
    Returns dict(rays (3,N,3) = [o, d, d], near (N,1), far (N,1), ray_mask (H*W,) bool) -- the per-frame entries a
    reference dataset yields (freeview.py:232-242).  One host sync (the ray count sizes the views).  ``camera_turn`` (3,3):
    the third row is M d instead of d -- the directions under the camera's extrinsics before the body's global transform
    (dataset.camera_turn; view-dependent colour with view_dir_camera_only)."""
    lib = _lib.load()
    import numpy as np
    device = device or torch.device('cuda', torch.cuda.current_device())
    K = np.asarray(K.cpu() if torch.is_tensor(K) else K, dtype=np.float32)
    E = np.asarray(E.cpu() if torch.is_tensor(E) else E, dtype=np.float32)
    small = np.concatenate([np.linalg.inv(K).reshape(-1), E[:3, :3].reshape(-1), E[:3, 3].reshape(-1),
                            np.asarray(bbox_min, np.float32).reshape(-1), np.asarray(bbox_max, np.float32).reshape(-1)])
    cam = torch.from_numpy(small.astype(np.float32)).to(device)
    n = H * W
    rays_o, rays_d = torch.empty(n, 3, device=device), torch.empty(n, 3, device=device)
    near, far = torch.empty(n, device=device), torch.empty(n, device=device)
    mask = torch.empty(n, dtype=torch.uint8, device=device)
    count = torch.empty(1, dtype=torch.int32, device=device)
    ws = torch.empty(lib.hnrf_gen_rays_workspace_bytes(H, W), dtype=torch.uint8, device=device)
    base = cam.data_ptr()
    _lib.check(lib.hnrf_gen_rays(base, base + 36, base + 72, base + 84, base + 96, H, W, _ptr(rays_o), _ptr(rays_d),
                                 _ptr(near), _ptr(far), mask.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _stream()), 'hnrf_gen_rays')
    N = int(count.item())
    o, d = rays_o[:N], rays_d[:N]
    dc = d
    if camera_turn is not None:
        dc = d @ torch.as_tensor(np.asarray(camera_turn.cpu() if torch.is_tensor(camera_turn) else camera_turn, dtype=np.float32),
                                 device=device).t()
    return {'rays': torch.stack([o, d, dc], 0), 'near': near[:N, None], 'far': far[:N, None], 'ray_mask': mask.bool()}


# ------------------------------------------------------------------------------------------------ image pre-processing
# (hnrf_image.hip; the host statement of the same OpenCV functions is imageproc.py)
_image_consts = {}                    # (kind, key..., device) -> device tensors built once per camera / image size


def _upload(arr, device):
    """Small host array -> device through pinned memory (a pageable copy would wait for the stream's queue)."""
    t = torch.from_numpy(arr)
    return t.pin_memory().to(device, non_blocking=True) if torch.device(device).type == 'cuda' else t.to(device)


def _u8_image(t, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3):
        raise _lib.HnrfError('%s must be a contiguous uint8 (H, W, C) tensor on the GPU' % what)


def undistort_image(img, K, D):
    """cv2.undistort(img, K, D) (train.py:366-371) of a uint8 (H, W, C) image on the device -> new tensor.  K (3,3),
    D (5,) host arrays; the per-camera constants (stripe inverses) are uploaded once per camera and image size."""
    import numpy as np
    from . import imageproc
    lib = _lib.load()
    _u8_image(img, 'undistort_image: img')
    H, W, C = img.shape
    A = np.asarray(K, dtype=np.float64)[:3, :3]
    d = imageproc.distortion_vector(D)
    key = ('undistort', A.tobytes(), d.tobytes(), H, W, img.device)
    c = _image_consts.get(key)
    if c is None:
        rows, ir = imageproc.undistort_stripes(A, H, W)
        cam = np.concatenate([[A[0, 0], A[1, 1], A[0, 2], A[1, 2]], d])
        c = _image_consts[key] = (_upload(cam, img.device), _upload(np.ascontiguousarray(ir), img.device), len(ir), rows)
    out = torch.empty_like(img)
    _lib.check(lib.hnrf_undistort_image(img.data_ptr(), H, W, C, c[0].data_ptr(), c[1].data_ptr(), c[2], c[3],
                                        out.data_ptr(), _stream()), 'hnrf_undistort_image')
    return out


def _resize_tables(Hs, Ws, scale, kind, device):
    import numpy as np
    from . import imageproc
    key = ('tables', Hs, Ws, float(scale), kind, device)
    t = _image_consts.get(key)
    if t is None:
        Hd, Wd = imageproc.resized_size(Hs, Ws, scale)
        inv = 1.0 / float(scale)
        xo, xw = imageproc.resize_tables(Ws, Wd, inv, kind)
        yo, yw = imageproc.resize_tables(Hs, Hd, inv, kind)
        t = _image_consts[key] = (Hd, Wd) + tuple(_upload(np.ascontiguousarray(a), device) for a in (xo, xw, yo, yw))
    return t


def composite_windows(orig, alpha, bgcolor, windows, ph, pw, scale=1.0):
    """float32 [n, ph, pw, 3] = pixels of ``load_image(...)[0] / 255`` (train.py:406-417: composite over ``bgcolor``
    (0..255, float32 [3] on the device), then INTER_LANCZOS4 to ``scale``) inside the n windows whose top-left
    destination pixels are ``windows`` ((n, 2) of (x0, y0): host ints, checked here).  orig / alpha: uint8 (Hs, Ws, 3)
    on the device, already undistorted.  One whole image = one window at (0, 0)."""
    import numpy as np
    from . import imageproc
    lib = _lib.load()
    _u8_image(orig, 'composite_windows: orig')
    _u8_image(alpha, 'composite_windows: alpha')
    _chk(bgcolor)
    Hs, Ws, C = orig.shape
    assert C == 3 and alpha.shape == orig.shape and bgcolor.numel() == 3
    win = np.ascontiguousarray(np.asarray(windows, dtype=np.int32).reshape(-1, 2))
    resize = 0 if float(scale) == 1.0 else 1
    if resize:
        Hd, Wd, xo, xw, yo, yw = _resize_tables(Hs, Ws, scale, 'lanczos4', orig.device)
    else:
        Hd, Wd, xo, xw, yo, yw = Hs, Ws, None, None, None, None
    if len(win) == 0 or win.min() < 0 or (win[:, 0] + pw).max() > Wd or (win[:, 1] + ph).max() > Hd:
        raise _lib.HnrfError('composite_windows: windows %s of %dx%d leave the %dx%d image' % (win.tolist(), ph, pw, Hd, Wd))
    win_d = _upload(win, orig.device)
    out = torch.empty(len(win), ph, pw, 3, device=orig.device)
    _lib.check(lib.hnrf_composite_windows(orig.data_ptr(), alpha.data_ptr(), Hs, Ws, bgcolor.data_ptr(), resize, _ptr(xo),
                                          _ptr(xw), _ptr(yo), _ptr(yw), Hd, Wd, win_d.data_ptr(), len(win), ph, pw,
                                          out.data_ptr(), _stream()), 'hnrf_composite_windows')
    return out


def resize_mask(alpha, scale, channel=0):
    """float32 (Hd, Wd): channel ``channel`` of ``cv2.resize(alpha / 255, fx=scale, fy=scale, INTER_LINEAR)``
    (train.py:413-417); at scale 1 the channel / 255 itself."""
    from . import imageproc
    lib = _lib.load()
    _u8_image(alpha, 'resize_mask: alpha')
    Hs, Ws, C = alpha.shape
    assert C == 3
    if float(scale) == 1.0:
        return (alpha[:, :, channel].double() / 255.).float()
    Hd, Wd = imageproc.resized_size(Hs, Ws, scale)
    out = torch.empty(Hd, Wd, device=alpha.device)
    if imageproc.is_half_scale(scale) and 2 * Hd <= Hs and 2 * Wd <= Ws:
        _lib.check(lib.hnrf_resize_mask(alpha.data_ptr(), Hs, Ws, channel, 2, 0, 0, 0, 0, Hd, Wd, out.data_ptr(), _stream()),
                   'hnrf_resize_mask')
    else:
        _, _, xo, xw, yo, yw = _resize_tables(Hs, Ws, scale, 'linear', alpha.device)
        _lib.check(lib.hnrf_resize_mask(alpha.data_ptr(), Hs, Ws, channel, 1, xo.data_ptr(), xw.data_ptr(), yo.data_ptr(),
                                        yw.data_ptr(), Hd, Wd, out.data_ptr(), _stream()), 'hnrf_resize_mask')
    return out


def deconv_fold(col, bias, cout, D, H, W):
    """hnrf_deconv_fold: col (D*H*W, cout*64) fp32 -> (1, cout, 2D, 2H, 2W): the fold of ConvTranspose3d(4, 2, 1)."""
    lib = _lib.load()
    _chk(col, bias)
    assert tuple(col.shape) == (D * H * W, cout * 64) and (bias is None or bias.numel() == cout)
    out = torch.empty(1, cout, 2 * D, 2 * H, 2 * W, device=col.device)
    _lib.check(lib.hnrf_deconv_fold(_ptr(col), _ptr(bias), cout, D, H, W, _ptr(out), _stream()), 'hnrf_deconv_fold')
    return out


def density_grid(packed, vol, bbox_min, bbox_max, bbox_scale, N, mode='f32', want_parts=False):
    """hnrf_density_grid: relu(sigma) * fg on the N^3 lattice over [bbox_min, bbox_max], (N, N, N) indexed [z][y][x].
    ``vol`` (B+1, G, G, G) with the background channel last (fg sums the B bone channels).  ``want_parts``: also
    return sigma and fg, each (N, N, N)."""
    lib = _lib.load()
    _chk(packed, vol, bbox_min, bbox_max, bbox_scale)
    N = int(N)
    B, G = vol.shape[0] - 1, vol.shape[-1]
    assert vol.dim() == 4 and vol.shape[1] == vol.shape[2] == G and B >= 1
    dev = vol.device
    need = lib.hnrf_density_grid_workspace_bytes(N)
    if need == 0:
        raise _lib.HnrfError(f'density grid resolution {N} out of range [8, 512]')
    ws = torch.empty(need // 4 + 64, device=dev)
    density = torch.empty(N, N, N, device=dev)
    sigma = torch.empty(N, N, N, device=dev) if want_parts else None
    fg = torch.empty(N, N, N, device=dev) if want_parts else None
    _lib.check(lib.hnrf_density_grid(_ptr(packed), _mode_arg(mode), _ptr(vol), B, G, _ptr(bbox_min), _ptr(bbox_max),
                                     _ptr(bbox_scale), N, _ptr(ws), ws.numel() * 4, _ptr(density), _ptr(sigma), _ptr(fg),
                                     _stream()), 'hnrf_density_grid')
    return (density, sigma, fg) if want_parts else density


# ------------------------------------------------------------------------------------------------ baked canonical grid
def _chk_grid(grid, bbox_min, bbox_max):
    """-> N of a baked grid: contiguous float16 (N, N, N, 4) on the GPU, with its fp32 box."""
    if not (torch.is_tensor(grid) and grid.is_cuda and grid.dtype == torch.float16 and grid.is_contiguous()
            and grid.dim() == 4 and grid.shape[0] == grid.shape[1] == grid.shape[2] and grid.shape[3] == 4):
        raise _lib.HnrfError('baked grid must be a contiguous float16 (N, N, N, 4) tensor on the GPU')
    _chk(bbox_min, bbox_max)
    assert bbox_min.numel() == 3 and bbox_max.numel() == 3
    return int(grid.shape[0])


def _baked_args(baked, device):
    """The four arguments that stand for cnl_packed in the *_baked_fwd entries."""
    grid, bbox_min, bbox_max = baked
    N = _chk_grid(grid, bbox_min, bbox_max)
    if grid.device != device:
        raise _lib.HnrfError(f'baked grid on {grid.device}, rays on {device}')
    return [grid.data_ptr(), N, _ptr(bbox_min), _ptr(bbox_max)]


def _chk_baked_nr(baked, baked_nr):
    if baked_nr is not None and baked is None:
        raise _lib.HnrfError('baked_nr (the offset grid) needs baked (the canonical grid): the two are sampled in one '
                             'kernel, and there is no offset grid in front of the canonical MLP')


def bake_canonical(packed, bbox_min, bbox_max, N, mode='f32', want_saturated=False):
    """hnrf_bake_canonical: the canonical MLP (``packed``, ``mode``) on the N^3 lattice over [bbox_min, bbox_max] ->
    grid (N, N, N, 4) float16 indexed [z][y][x][c], c = (r, g, b, sigma) pre-activation, values beyond +-65504
    saturated.  ``want_saturated``: also return their count, a (1,) int32 device tensor (no synchronisation)."""
    lib = _lib.load()
    _chk(packed, bbox_min, bbox_max)
    N = int(N)
    need = lib.hnrf_bake_canonical_workspace_bytes(N)
    if need == 0:
        raise _lib.HnrfError(f'baked grid resolution {N} out of range [8, 512]')
    dev = packed.device
    ws = torch.empty(need // 4 + 64, device=dev)
    grid = torch.empty(N, N, N, 4, dtype=torch.float16, device=dev)
    sat = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.hnrf_bake_canonical(_ptr(packed), _mode_arg(mode), _ptr(bbox_min), _ptr(bbox_max), N, _ptr(ws),
                                       ws.numel() * 4, grid.data_ptr(), sat.data_ptr(), _stream()), 'hnrf_bake_canonical')
    return (grid, sat) if want_saturated else grid


def baked_sample(xyz, grid, bbox_min, bbox_max):
    """hnrf_baked_sample: xyz (..., 3) -> raw (..., 4), the grid interpolated where ``canonical`` runs the MLP."""
    lib = _lib.load()
    _chk(xyz)
    N = _chk_grid(grid, bbox_min, bbox_max)
    raw = torch.empty(*xyz.shape[:-1], 4, device=xyz.device)
    _lib.check(lib.hnrf_baked_sample(_ptr(xyz), grid.data_ptr(), N, _ptr(bbox_min), _ptr(bbox_max), xyz.numel() // 3,
                                     _ptr(raw), _stream()), 'hnrf_baked_sample')
    return raw


def baked_sample_sparse(xyz, grid, bbox_min, bbox_max, idx, count, raw=None):
    """hnrf_baked_sample_sparse: only the samples idx[0 .. count) are read and written; ``raw`` (default zeros) keeps
    its other rows."""
    lib = _lib.load()
    _chk(xyz, raw)
    N = _chk_grid(grid, bbox_min, bbox_max)
    if raw is None:
        raw = torch.zeros(*xyz.shape[:-1], 4, device=xyz.device)
    assert raw.numel() // 4 == xyz.numel() // 3
    _lib.check(lib.hnrf_baked_sample_sparse(_ptr(xyz), grid.data_ptr(), N, _ptr(bbox_min), _ptr(bbox_max),
                                            xyz.numel() // 3, _ptr(idx), _ptr(count), _ptr(raw), _stream()),
               'hnrf_baked_sample_sparse')
    return raw


# ---------------------------------------------------------------------------------- baked non-rigid offset field
def bake_nonrigid_workspace(M, device):
    """A workspace for bake_nonrigid at resolution M (a per-frame caller keeps it)."""
    need = _lib.load().hnrf_bake_nonrigid_workspace_bytes(int(M))
    if need == 0:
        raise _lib.HnrfError(f'offset grid resolution {M} out of range [8, 512]')
    return torch.empty(need // 4 + 64, device=device)


def bake_nonrigid(nr_packed, hann_w, bbox_min, bbox_max, M, mode='f32', want_saturated=False, workspace=None, out=None):
    """hnrf_bake_nonrigid: the offsets of the non-rigid MLP (``nr_packed`` -- one frame's condition code folded in --,
    ``hann_w``, ``mode``) on the M^3 lattice over [bbox_min, bbox_max] -> grid (M, M, M, 4) float16 indexed
    [z][y][x][c], c = (dx, dy, dz, +0), values beyond +-65504 saturated.  ``want_saturated``: also return their count, a
    (1,) int32 device tensor (no synchronisation).  ``workspace`` (bake_nonrigid_workspace) / ``out`` (a grid tensor):
    buffers of a per-frame caller to use instead of fresh ones."""
    lib = _lib.load()
    _chk(nr_packed, hann_w, bbox_min, bbox_max, workspace)
    M = int(M)
    dev = nr_packed.device
    ws = workspace if workspace is not None else bake_nonrigid_workspace(M, dev)
    grid = out if out is not None else torch.empty(M, M, M, 4, dtype=torch.float16, device=dev)
    if _chk_grid(grid, bbox_min, bbox_max) != M or grid.device != dev or ws.device != dev:
        raise _lib.HnrfError(f'bake_nonrigid: out must be a ({M}, {M}, {M}, 4) grid on {dev}')
    sat = torch.zeros(1, dtype=torch.int32, device=dev) if want_saturated else None
    _lib.check(lib.hnrf_bake_nonrigid(_ptr(nr_packed), _ptr(hann_w), _mode_arg(mode), _ptr(bbox_min), _ptr(bbox_max), M,
                                      _ptr(ws), ws.numel() * 4, grid.data_ptr(), _ptr(sat), _stream()),
               'hnrf_bake_nonrigid')
    return (grid, sat) if want_saturated else grid


def _warp_sample_args(x_skel, off, cnl, want_xyz, want_offsets):
    _chk(x_skel)
    M = _chk_grid(*off)
    N = _chk_grid(*cnl)
    dev = x_skel.device
    if off[0].device != dev or cnl[0].device != dev:
        raise _lib.HnrfError(f'baked grids on {off[0].device} / {cnl[0].device}, samples on {dev}')
    xyz = torch.empty_like(x_skel) if want_xyz else None
    offsets = torch.empty_like(x_skel) if want_offsets else None
    args = [_ptr(x_skel), off[0].data_ptr(), M, _ptr(off[1]), _ptr(off[2]), cnl[0].data_ptr(), N, _ptr(cnl[1]),
            _ptr(cnl[2]), x_skel.numel() // 3]
    return args, xyz, offsets


def baked_warp_sample(x_skel, off, cnl, want_xyz=False, want_offsets=False):
    """hnrf_baked_warp_sample: x_skel (..., 3) -> raw (..., 4) = the canonical grid ``cnl`` = (grid, bbox_min, bbox_max)
    sampled at xyz = x_skel + the offset grid ``off`` = (off_grid, bbox_min, bbox_max) sampled at x_skel: one kernel for
    the chain baked_sample -> add -> baked_sample.  Returns raw, or (raw, xyz or None, offsets or None) when either is
    asked for."""
    lib = _lib.load()
    args, xyz, offsets = _warp_sample_args(x_skel, off, cnl, want_xyz, want_offsets)
    raw = torch.empty(*x_skel.shape[:-1], 4, device=x_skel.device)
    _lib.check(lib.hnrf_baked_warp_sample(*args, _ptr(raw), _ptr(xyz), _ptr(offsets), _stream()), 'hnrf_baked_warp_sample')
    return (raw, xyz, offsets) if (want_xyz or want_offsets) else raw


def baked_warp_sample_sparse(x_skel, off, cnl, idx, count, raw=None, xyz=None, offsets=None):
    """hnrf_baked_warp_sample_sparse: only the samples idx[0 .. count) are read and written; ``raw`` (default zeros)
    and the optional ``xyz`` / ``offsets`` tensors (of x_skel's shape) keep their other rows.  Returns raw."""
    lib = _lib.load()
    _chk(raw, xyz, offsets)
    args, _, _ = _warp_sample_args(x_skel, off, cnl, False, False)
    if raw is None:
        raw = torch.zeros(*x_skel.shape[:-1], 4, device=x_skel.device)
    assert raw.numel() // 4 == x_skel.numel() // 3
    assert all(t is None or t.numel() == x_skel.numel() for t in (xyz, offsets))
    _lib.check(lib.hnrf_baked_warp_sample_sparse(*args, _ptr(idx), _ptr(count), _ptr(raw), _ptr(xyz), _ptr(offsets),
                                                 _stream()), 'hnrf_baked_warp_sample_sparse')
    return raw


def mesh_workspace(N, device):
    need = _lib.load().hnrf_mesh_workspace_bytes(int(N))
    if need == 0:
        raise _lib.HnrfError(f'mesh lattice resolution {N} out of range [8, 512]')
    return torch.empty(need // 4 + 64, device=device)


def mesh_count(density, level, workspace):
    """hnrf_mesh_count: density (N, N, N) -> (V, F) on the host (one synchronisation); fills ``workspace``."""
    lib = _lib.load()
    _chk(density, workspace)
    N = density.shape[0]
    assert density.shape == (N, N, N)
    counts = torch.empty(2, dtype=torch.int64, device=density.device)
    _lib.check(lib.hnrf_mesh_count(_ptr(density), N, float(level), _ptr(workspace), workspace.numel() * 4, _ptr(counts),
                                   _stream()), 'hnrf_mesh_count')
    V, F = (int(v) for v in counts.cpu())
    return V, F


def mesh_emit(density, level, bbox_min, bbox_max, workspace, V, F):
    """hnrf_mesh_emit after mesh_count on the same density / level / workspace: verts (V, 3) fp32, faces (F, 3) int32."""
    lib = _lib.load()
    _chk(density, bbox_min, bbox_max, workspace)
    N = density.shape[0]
    if V >= 2 ** 31:
        raise _lib.HnrfError(f'{V} mesh vertices: int32 vertex ids hold at most 2^31 - 1')
    verts = torch.empty(V, 3, device=density.device)
    faces = torch.empty(F, 3, dtype=torch.int32, device=density.device)
    _lib.check(lib.hnrf_mesh_emit(_ptr(density), N, float(level), _ptr(bbox_min), _ptr(bbox_max), _ptr(workspace),
                                  workspace.numel() * 4, V, F, _ptr(verts), _ptr(faces), _stream()), 'hnrf_mesh_emit')
    return verts, faces


def forward_skin(verts, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale):
    """hnrf_forward_skin: canonical verts (V, 3) -> posed (V, 3) under the motion basis (B,3,3), (B,3)."""
    lib = _lib.load()
    _chk(verts, motion_Rs, motion_Ts, vol, bbox_min, bbox_scale)
    B, G = motion_Rs.shape[0], vol.shape[-1]
    assert vol.shape[0] >= B and verts.shape[-1] == 3
    out = torch.empty_like(verts)
    _lib.check(lib.hnrf_forward_skin(_ptr(verts), verts.shape[0], _ptr(motion_Rs), _ptr(motion_Ts), _ptr(vol), B, G,
                                     _ptr(bbox_min), _ptr(bbox_scale), _ptr(out), _stream()), 'hnrf_forward_skin')
    return out


def _chk_skin_k(k):
    k = int(k)
    if k not in (4, 8):
        raise _lib.HnrfError(f'{k} influences per vertex: glTF skinning is built for 4 or 8')
    return k


def skin_weights(verts, vol, n_bones, bbox_min, bbox_scale, k=4):
    """hnrf_skin_weights: the k largest of the first ``n_bones`` channels of vol at verts (V, 3), normalised ->
    joints (V, k) uint8, weights (V, k) fp32, kept (V,) fp32 (the sum of the selected weights)."""
    lib = _lib.load_skin()
    _chk(verts, vol, bbox_min, bbox_scale)
    k, B, G, V = _chk_skin_k(k), int(n_bones), vol.shape[-1], verts.shape[0]
    assert vol.shape[0] >= B and verts.dim() == 2 and verts.shape[1] == 3
    joints = torch.empty(V, k, dtype=torch.uint8, device=verts.device)
    weights = torch.empty(V, k, device=verts.device)
    kept = torch.empty(V, device=verts.device)
    _lib.check(lib.hnrf_skin_weights(_ptr(verts), V, _ptr(vol), B, G, _ptr(bbox_min), _ptr(bbox_scale), k, _ptr(joints),
                                     _ptr(weights), _ptr(kept), _stream()), 'hnrf_skin_weights')
    return joints, weights, kept


def skin_lbs(verts, joints, weights, mats):
    """hnrf_skin_lbs: out (V, 3) = sum_k weights[:, k] (mats[joints[:, k]] (x, 1)); mats (B, 3, 4)."""
    lib = _lib.load_skin()
    _chk(verts, weights, mats)
    _chk_dev(joints, torch.uint8, 'joints')
    V, k = verts.shape[0], _chk_skin_k(weights.shape[-1])
    assert verts.dim() == 2 and verts.shape[1] == 3 and tuple(joints.shape) == (V, k) == tuple(weights.shape)
    assert mats.dim() == 3 and tuple(mats.shape[1:]) == (3, 4)
    out = torch.empty_like(verts)
    _lib.check(lib.hnrf_skin_lbs(_ptr(verts), V, _ptr(joints), _ptr(weights), k, _ptr(mats), mats.shape[0], _ptr(out),
                                 _stream()), 'hnrf_skin_lbs')
    return out


_raster_ws = {}                       # (V, F, H, W, device) -> workspace of the last call of that shape


def raster_workspace(V, F, H, W, device):
    """Workspace of hnrf_raster_mesh, kept per shape (a frame loop rasterises one mesh into one image size)."""
    key = (int(V), int(F), int(H), int(W), torch.device(device))
    ws = _raster_ws.get(key)
    if ws is None:
        need = _lib.load().hnrf_raster_workspace_bytes(int(V), int(F), int(H), int(W))
        if need == 0:
            raise _lib.HnrfError(f'raster: V={V} F={F} image {H}x{W} out of range')
        if len(_raster_ws) >= 8:
            _raster_ws.clear()
        ws = _raster_ws[key] = torch.empty(need // 4 + 64, device=device)
    return ws


def raster_mesh(verts, faces, colors, cam, H, W, z_near, flags):
    """hnrf_raster_mesh: verts (V, 3) fp32, faces (F, 3) int32, colors (V, 3) fp32 or None (shade normal), ``cam`` the
    24 floats K | R | T | bgcolor on the device, ``flags`` cull | shade (hnrf.h).  Returns dict(rgb (H, W, 3), alpha,
    depth (H, W), tri_id (H, W) int32).  No synchronisation."""
    lib = _lib.load()
    _chk(verts, colors, cam)
    if not (faces.is_cuda and faces.dtype == torch.int32 and faces.is_contiguous()):
        raise _lib.HnrfError('raster_mesh: faces must be a contiguous int32 tensor on the GPU')
    assert verts.dim() == 2 and verts.shape[1] == 3 and faces.dim() == 2 and faces.shape[1] == 3 and cam.numel() == 24
    assert colors is None or colors.shape == verts.shape
    dev = verts.device
    V, F = verts.shape[0], faces.shape[0]
    ws = raster_workspace(V, F, H, W, dev)
    out = {'rgb': torch.empty(H, W, 3, device=dev), 'alpha': torch.empty(H, W, device=dev),
           'depth': torch.empty(H, W, device=dev), 'tri_id': torch.empty(H, W, dtype=torch.int32, device=dev)}
    base = cam.data_ptr()
    _lib.check(lib.hnrf_raster_mesh(_ptr(verts), V, faces.data_ptr(), F, _ptr(colors), base, base + 36, base + 72,
                                    base + 84, H, W, float(z_near), int(flags), _ptr(out['rgb']), _ptr(out['alpha']),
                                    _ptr(out['depth']), out['tri_id'].data_ptr(), _ptr(ws), ws.numel() * 4, _stream()),
               'hnrf_raster_mesh')
    return out


# ------------------------------------------------------------------------------------------------------------ LPIPS
LPIPS_CONVS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512),
               (512, 512), (512, 512), (512, 512), (512, 512)]       # (Cin, Cout) of trunk layers 0..12 (hnrf.h)
LPIPS_TAPS = [(1, 64), (3, 128), (6, 256), (9, 512), (12, 512)]      # (layer, channels) of the five taps


def _aligned(nbytes, device):
    """Uninitialised fp32 buffer of at least ``nbytes`` whose data pointer is 256-byte aligned."""
    t = torch.empty(nbytes // 4 + 64, device=device)
    off = (-t.data_ptr() % 256) // 4
    return t[off:off + (nbytes + 3) // 4]


def lpips_pack(weights, biases, lins):
    """hnrf_lpips_pack: the 13 (Cout,Cin,3,3) weights, 13 biases and 5 head vectors -> the packed image."""
    lib = _lib.load()
    lins = [v.reshape(-1) for v in lins]
    _chk(*weights, *biases, *lins)
    assert len(weights) == 13 and len(biases) == 13 and len(lins) == 5
    for w, b, (ci, co) in zip(weights, biases, LPIPS_CONVS):
        assert tuple(w.shape) == (co, ci, 3, 3) and b.numel() == co, (tuple(w.shape), (co, ci, 3, 3))
    for v, (_, c) in zip(lins, LPIPS_TAPS):
        assert v.numel() == c
    out = _aligned(lib.hnrf_lpips_packed_bytes(), weights[0].device)
    _lib.check(lib.hnrf_lpips_pack(_ptr_array(weights), _ptr_array(biases), _ptr_array(lins), _ptr(out), _stream()),
               'hnrf_lpips_pack')
    return out


def conv3x3_fwd(x, packed, layer, scale_input=False, out=None):
    """hnrf_conv3x3_fwd: x (N,H,W,Cin) -> relu(conv + bias) (N,H,W,Cout) of trunk layer ``layer``."""
    lib = _lib.load()
    _chk(x, packed, out)
    N, H, W, C = x.shape
    assert C == LPIPS_CONVS[layer][0]
    y = out if out is not None else torch.empty(N, H, W, LPIPS_CONVS[layer][1], device=x.device)
    _lib.check(lib.hnrf_conv3x3_fwd(_ptr(x), _ptr(packed), int(layer), N, H, W, int(bool(scale_input)), _ptr(y),
                                    _stream()), 'hnrf_conv3x3_fwd')
    return y


def conv3x3_bwd_data(dy, y_saved, packed, layer, unscale_output=False, out=None):
    """hnrf_conv3x3_bwd_data: dy (N,H,W,Cout) [masked by y_saved > 0] -> dx (N,H,W,Cin)."""
    lib = _lib.load()
    _chk(dy, y_saved, packed, out)
    N, H, W, C = dy.shape
    assert C == LPIPS_CONVS[layer][1] and (y_saved is None or y_saved.shape == dy.shape)
    dx = out if out is not None else torch.empty(N, H, W, LPIPS_CONVS[layer][0], device=dy.device)
    _lib.check(lib.hnrf_conv3x3_bwd_data(_ptr(dy), _ptr(y_saved), _ptr(packed), int(layer), N, H, W,
                                         int(bool(unscale_output)), _ptr(dx), _stream()), 'hnrf_conv3x3_bwd_data')
    return dx


def maxpool2_fwd(x, out=None):
    """hnrf_maxpool2_fwd: (N,H,W,C) -> (N,H//2,W//2,C)."""
    lib = _lib.load()
    _chk(x, out)
    N, H, W, C = x.shape
    y = out if out is not None else torch.empty(N, H // 2, W // 2, C, device=x.device)
    _lib.check(lib.hnrf_maxpool2_fwd(_ptr(x), N, H, W, C, _ptr(y), _stream()), 'hnrf_maxpool2_fwd')
    return y


def maxpool2_bwd(x, dy, out=None):
    """hnrf_maxpool2_bwd: the gradient of maxpool2_fwd(x) with respect to x."""
    lib = _lib.load()
    _chk(x, dy, out)
    N, H, W, C = x.shape
    assert dy.shape == (N, H // 2, W // 2, C)
    dx = out if out is not None else torch.empty_like(x)
    _lib.check(lib.hnrf_maxpool2_bwd(_ptr(x), _ptr(dy), N, H, W, C, _ptr(dx), _stream()), 'hnrf_maxpool2_bwd')
    return dx


def lpips_head_fwd(f, w, out=None, accumulate=False, pix=None):
    """hnrf_lpips_head_fwd: f (2N,P,C) (first the N maps of image 0, then those of image 1), w (C) -> (out (N), v (N))."""
    lib = _lib.load()
    _chk(f, w, out, pix)
    B, P, C = f.shape
    N = B // 2
    assert B == 2 * N and w.numel() == C
    pix = pix if pix is not None else torch.empty(max(N * P, 1), device=f.device)
    out = out if out is not None else torch.empty(N, device=f.device)
    val = torch.empty(N, device=f.device)
    _lib.check(lib.hnrf_lpips_head_fwd(_ptr(f), _ptr(w), N, P, C, _ptr(pix), _ptr(out), int(bool(accumulate)),
                                       _ptr(val), _stream()), 'hnrf_lpips_head_fwd')
    return out, val


def lpips_head_bwd(f, w, grad_out, out=None, accumulate=False):
    """hnrf_lpips_head_bwd: d/d f[:N] of sum_n grad_out[n] v[n] -> (N,P,C), added to ``out`` when ``accumulate``."""
    lib = _lib.load()
    _chk(f, w, grad_out, out)
    B, P, C = f.shape
    N = B // 2
    assert B == 2 * N and w.numel() == C and grad_out.numel() == N
    dx = out if out is not None else torch.empty(N, P, C, device=f.device)
    _lib.check(lib.hnrf_lpips_head_bwd(_ptr(f), _ptr(w), _ptr(grad_out), N, P, C, _ptr(dx), int(bool(accumulate)),
                                       _stream()), 'hnrf_lpips_head_bwd')
    return dx


def lpips_workspace(N, H, W, want_grad, device):
    need = _lib.load().hnrf_lpips_workspace_bytes(int(N), int(H), int(W), int(bool(want_grad)))
    if need == 0:
        raise _lib.HnrfError(f'lpips: N={N} images of {H}x{W} refused (H, W >= 16, 2*N*H*W*64 < 2^31)')
    return _aligned(need, device)


def lpips_fwd(img0, img1, packed, want_grad=False, workspace=None, want_layers=False):
    """hnrf_lpips_fwd: img0, img1 (N,H,W,3) in [-1, 1] -> (value (N), per-tap values (5,N) or None, workspace)."""
    lib = _lib.load()
    _chk(img0, img1, packed, workspace)
    N, H, W, C = img0.shape
    assert C == 3 and img1.shape == img0.shape
    ws = workspace if workspace is not None else lpips_workspace(N, H, W, want_grad, img0.device)
    out = torch.empty(N, device=img0.device)
    per = torch.empty(5, N, device=img0.device) if want_layers else None
    _lib.check(lib.hnrf_lpips_fwd(_ptr(img0), _ptr(img1), _ptr(packed), N, H, W, int(bool(want_grad)), _ptr(ws),
                                  ws.numel() * 4, _ptr(out), _ptr(per), _stream()), 'hnrf_lpips_fwd')
    return out, per, ws


def lpips_bwd(grad_out, packed, workspace, N, H, W):
    """hnrf_lpips_bwd on the workspace of lpips_fwd(..., want_grad=True): -> d img0 (N,H,W,3)."""
    lib = _lib.load()
    _chk(grad_out, packed, workspace)
    assert grad_out.numel() == N
    d = torch.empty(N, H, W, 3, device=grad_out.device)
    _lib.check(lib.hnrf_lpips_bwd(_ptr(grad_out), _ptr(packed), N, H, W, _ptr(workspace), workspace.numel() * 4,
                                  _ptr(d), _stream()), 'hnrf_lpips_bwd')
    return d


# ---------------------------------------------------------------------------------------------------- image metrics
_metrics_ws = {}                      # (n, H, W, device) -> workspace of the last call of that shape


def image_metrics_workspace(n, H, W, device):
    """Workspace of hnrf_image_metrics, kept per shape (a frame loop compares one image size); calls that share it
    must be ordered on one stream."""
    key = (int(n), int(H), int(W), torch.device(device))
    ws = _metrics_ws.get(key)
    if ws is None:
        need = _lib.load().hnrf_image_metrics_workspace_bytes(int(n), int(H), int(W))
        if need == 0:
            raise _lib.HnrfError(f'image_metrics: {n} images of {H}x{W} out of range')
        if len(_metrics_ws) >= 8:
            _metrics_ws.clear()
        ws = _metrics_ws[key] = _aligned(need, device)
    return ws


def image_metrics(pred8, target8, mask=None, data_range=1.0):
    """hnrf_image_metrics: PSNR and SSIM (render.psnr / render.ssim; render.metrics_u8 is the numpy twin) of uint8
    images on the device, (H, W, 3) or (N, H, W, 3); ``mask`` (H, W), (H, W, 1) or (N, H, W[, 1]) uint8 / bool, non-zero
    = inside.  Returns a float64 device tensor (n, 2): psnr, ssim per image.  No synchronisation; anything that is not
    uint8 on the GPU raises."""
    lib = _lib.load()
    for t, what in ((pred8, 'pred8'), (target8, 'target8')):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8):
            raise _lib.HnrfError('image_metrics: %s must be a uint8 tensor on the GPU (float images go through '
                                 'MetricsWriter.append)' % what)
    if pred8.dim() == 3:
        pred8, target8 = pred8[None], target8[None]
        mask = None if mask is None else mask[None]
    if pred8.dim() != 4 or pred8.shape[3] != 3 or target8.shape != pred8.shape:
        raise _lib.HnrfError('image_metrics: images must be (H, W, 3) or (N, H, W, 3) of one shape, got %s and %s'
                             % (tuple(pred8.shape), tuple(target8.shape)))
    n, H, W, _ = pred8.shape
    pred8, target8 = pred8.contiguous(), target8.contiguous()
    if mask is not None:
        if not (torch.is_tensor(mask) and mask.is_cuda and mask.dtype in (torch.uint8, torch.bool)):
            raise _lib.HnrfError('image_metrics: mask must be a uint8 or bool tensor on the GPU')
        if mask.numel() != n * H * W:
            raise _lib.HnrfError('image_metrics: mask %s does not fit %d images of %dx%d' % (tuple(mask.shape), n, H, W))
        mask = mask.reshape(n, H, W).contiguous().view(torch.uint8)
    with torch.cuda.device(pred8.device):
        ws = image_metrics_workspace(n, H, W, pred8.device)
        out = torch.empty(n, 2, dtype=torch.float64, device=pred8.device)
        _lib.check(lib.hnrf_image_metrics(pred8.data_ptr(), target8.data_ptr(), _ptr(mask), n, H, W, float(data_range),
                                          ws.data_ptr(), ws.numel() * 4, out.data_ptr(), _stream()), 'hnrf_image_metrics')
    return out


# ------------------------------------------------------------------------------- surface points and frame distance
def _chk_dev(t, dtype, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise _lib.HnrfError('%s must be a contiguous %s tensor on the GPU, got %s' % (
            what, dtype, (t.dtype, t.device, tuple(t.shape)) if torch.is_tensor(t) else type(t)))


def surface_points(weights, xyz, bmw):
    """hnrf_surface_points: weights (R, S), xyz (R, S, 3), bmw (R, S, B) -> wxyz (R, 3), wmax (R,), lbs (R,) int32."""
    lib = _lib.load_cloud()
    _chk(weights, xyz, bmw)
    if weights.dim() != 2 or xyz.shape != weights.shape + (3,) or bmw.dim() != 3 or bmw.shape[:2] != weights.shape:
        raise _lib.HnrfError('surface_points: weights (R, S), xyz (R, S, 3), bmw (R, S, B) expected, got %s %s %s'
                             % (tuple(weights.shape), tuple(xyz.shape), tuple(bmw.shape)))
    R, S = weights.shape
    dev = weights.device
    wxyz, wmax = torch.empty(R, 3, device=dev), torch.empty(R, device=dev)
    lbs = torch.empty(R, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.hnrf_surface_points(_ptr(weights), _ptr(xyz), _ptr(bmw), R, S, int(bmw.shape[2]), _ptr(wxyz),
                                           _ptr(wmax), _ptr(lbs), _stream()), 'hnrf_surface_points')
    return wxyz, wmax, lbs


def cloud_nn(a, b, idx=None, d2=None):
    """hnrf_cloud_nn: a (Na, 3), b (Nb, 3) -> idx (Na,) int32, d2 (Na,): the nearest neighbour of every a in b (brute
    force; ties to the lowest index).  ``idx`` / ``d2``: outputs of at least Na elements to write into."""
    lib = _lib.load_cloud()
    _chk(a, b, d2)
    if a.dim() != 2 or a.shape[1] != 3 or b.dim() != 2 or b.shape[1] != 3:
        raise _lib.HnrfError('cloud_nn: clouds must be (N, 3), got %s and %s' % (tuple(a.shape), tuple(b.shape)))
    Na, Nb = a.shape[0], b.shape[0]
    idx = torch.empty(Na, dtype=torch.int32, device=a.device) if idx is None else idx
    d2 = torch.empty(Na, device=a.device) if d2 is None else d2
    _chk_dev(idx, torch.int32, 'cloud_nn: idx')
    if idx.numel() < Na or d2.numel() < Na:
        raise _lib.HnrfError('cloud_nn: outputs of %d / %d elements for %d points' % (idx.numel(), d2.numel(), Na))
    with torch.cuda.device(a.device):
        _lib.check(lib.hnrf_cloud_nn(_ptr(a), Na, _ptr(b), Nb, _ptr(idx), _ptr(d2), _stream()), 'hnrf_cloud_nn')
    return idx, d2


def cloud_distance_pairs(xyz, rgb, orig, offsets, pairs, tau, axis, max_n, want_match=False):
    """hnrf_cloud_distance_pairs on packed, per-frame sorted clouds (include/hnrf_cloud.h): xyz, rgb (total, 3), orig
    (total,) int32, offsets (F + 1,) int64, pairs (P, 2) int32, all on the GPU; ``max_n`` >= every frame's count.
    Returns D (P,) float64 and, with ``want_match``, match (P, max_n) int32 (else None)."""
    lib = _lib.load_cloud()
    _chk(xyz, rgb)
    _chk_dev(orig, torch.int32, 'cloud_distance_pairs: orig')
    _chk_dev(offsets, torch.int64, 'cloud_distance_pairs: offsets')
    _chk_dev(pairs, torch.int32, 'cloud_distance_pairs: pairs')
    total = xyz.shape[0]
    if xyz.dim() != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape or orig.shape != (total,):
        raise _lib.HnrfError('cloud_distance_pairs: xyz, rgb (total, 3) and orig (total,) expected, got %s %s %s'
                             % (tuple(xyz.shape), tuple(rgb.shape), tuple(orig.shape)))
    if offsets.dim() != 1 or offsets.numel() < 1 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise _lib.HnrfError('cloud_distance_pairs: offsets (F + 1,) and pairs (P, 2) expected, got %s %s'
                             % (tuple(offsets.shape), tuple(pairs.shape)))
    F, P, max_n = offsets.numel() - 1, pairs.shape[0], int(max_n)
    dev = xyz.device
    D = torch.empty(P, dtype=torch.float64, device=dev)
    match = torch.empty(P, max_n, dtype=torch.int32, device=dev) if want_match else None
    with torch.cuda.device(dev):
        need = lib.hnrf_cloud_distance_pairs_workspace_bytes(P, max_n)
        if need == 0:
            raise _lib.HnrfError('cloud_distance_pairs: %d pairs of at most %d points out of range' % (P, max_n))
        ws = _aligned(need, dev)
        _lib.check(lib.hnrf_cloud_distance_pairs(_ptr(xyz), _ptr(rgb), _ptr(orig), _ptr(offsets), F, total, _ptr(pairs), P,
                                                 max_n, int(axis), float(tau), ws.data_ptr(), ws.numel() * 4, _ptr(D),
                                                 _ptr(match), _stream()), 'hnrf_cloud_distance_pairs')
    return D, match


# ----------------------------------------------------------------------------------- body-part segmentation of records
SEGMENT_STATUS = {1: 'a row or column that is not integer-valued', 2: 'a pixel outside the image',
                  4: 'a bone index that is not integer-valued'}


def _segment_status(word, what):
    if word:
        raise _lib.HnrfError('%s: the records hold %s (status %d); nothing was written' % (
            what, ', '.join(v for k, v in SEGMENT_STATUS.items() if word & k) or 'an unknown fault', word))


def segment_members(rec, offsets, bone_masks, H, W, radius, member=None, status=None, frames_per_batch=None,
                    workspace_bytes=256 << 20):
    """hnrf_segment_members (include/hnrf_segment.h): rec (total, 10), offsets (F + 1,) int64 and bone_masks (B,) int32
    (the uint32 words) on the GPU -> member (total,) int32 (the uint32 words) and status (1,) int32, both device
    tensors: the status is NOT read back here (segment_compact does, with the counts).  Frames go through in batches
    whose bitmaps fit ``workspace_bytes`` (``frames_per_batch`` overrides); ``offsets`` must then be ascending."""
    lib = _lib.load_segment()
    _chk(rec)
    _chk_dev(offsets, torch.int64, 'segment_members: offsets')
    _chk_dev(bone_masks, torch.int32, 'segment_members: bone_masks')
    if rec.dim() != 2 or rec.shape[1] != 10 or offsets.dim() != 1 or offsets.numel() < 1 or bone_masks.dim() != 1:
        raise _lib.HnrfError('segment_members: rec (total, 10), offsets (F + 1,), bone_masks (B,) expected, got %s %s %s'
                             % (tuple(rec.shape), tuple(offsets.shape), tuple(bone_masks.shape)))
    total, F, dev = rec.shape[0], offsets.numel() - 1, rec.device
    H, W, radius = int(H), int(W), int(radius)
    member = torch.empty(total, dtype=torch.int32, device=dev) if member is None else member
    status = torch.zeros(1, dtype=torch.int32, device=dev) if status is None else status
    _chk_dev(member, torch.int32, 'segment_members: member')
    _chk_dev(status, torch.int32, 'segment_members: status')
    if member.numel() < total or status.numel() < 1:
        raise _lib.HnrfError('segment_members: member of %d elements for %d records' % (member.numel(), total))
    with torch.cuda.device(dev):
        per = lib.hnrf_segment_workspace_bytes(1, H, W)
        if frames_per_batch is None:
            frames_per_batch = max(1, int(workspace_bytes) // per) if per else max(F, 1)
        nb = max(1, min(int(frames_per_batch), F))
        need = lib.hnrf_segment_workspace_bytes(nb, H, W)
        ws = _aligned(max(need, 256), dev)

        def launch(r, o, n_frames, m, st):
            _lib.check(lib.hnrf_segment_members(_ptr(r), _ptr(o), n_frames, r.shape[0], _ptr(bone_masks),
                                                bone_masks.numel(), H, W, radius, ws.data_ptr(), ws.numel() * 4, _ptr(m),
                                                _ptr(st), _stream()), 'hnrf_segment_members')
        if nb >= F:
            launch(rec, offsets, F, member, status)
            return member, status
        host = offsets.cpu()                      # (the batches' row ranges: sizes the host side built itself)
        word = torch.zeros(1, dtype=torch.int32, device=dev)
        status.zero_()
        for f0 in range(0, F, nb):
            f1 = min(f0 + nb, F)
            r0, r1 = int(host[f0]), int(host[f1])
            launch(rec[r0:r1], (offsets[f0:f1 + 1] - r0).contiguous(), f1 - f0, member[r0:r1], word)
            status |= word
    return member, status


def segment_compact(member, offsets, n_parts, status=None, weight_rec=None, weight_min=0.0):
    """hnrf_segment_count + hnrf_segment_scatter: member (total,) int32, offsets (F + 1,) int64 -> seg_offsets
    (P F + 1,) int64 on the HOST (part-major) and src (rows,) int32 on the device.  With ``weight_rec`` (total, 10) only
    the records whose column 6 is > ``weight_min`` are kept.  One wait: the counts and the status word come back in one
    copy, and a status that is not 0 raises HnrfError before src exists."""
    lib = _lib.load_segment()
    _chk(weight_rec)
    _chk_dev(member, torch.int32, 'segment_compact: member')
    _chk_dev(offsets, torch.int64, 'segment_compact: offsets')
    total, F, P, dev = member.numel(), offsets.numel() - 1, int(n_parts), member.device
    if status is not None:
        _chk_dev(status, torch.int32, 'segment_compact: status')
    if weight_rec is not None and tuple(weight_rec.shape) != (total, 10):
        raise _lib.HnrfError('segment_compact: weight_rec %s for %d records' % (tuple(weight_rec.shape), total))
    with torch.cuda.device(dev):
        need = lib.hnrf_segment_compact_workspace_bytes(total, P)
        if need == 0:
            raise _lib.HnrfError('segment_compact: %d records in %d parts out of range (1 .. 32 parts)' % (total, P))
        ws = _aligned(need, dev)
        seg = torch.empty(max(P, 0) * F + 1, dtype=torch.int64, device=dev)
        _lib.check(lib.hnrf_segment_count(_ptr(member), _ptr(weight_rec), float(weight_min), _ptr(offsets), F, total, P,
                                          _ptr(status), ws.data_ptr(), ws.numel() * 4, _ptr(seg), _stream()),
                   'hnrf_segment_count')
        if status is None:
            seg_host = seg.cpu()
        else:                                                             # one copy, one wait
            both = torch.cat([seg, status[:1].to(torch.int64)]).cpu()
            _segment_status(int(both[-1]), 'segment_compact')              # (seg is unwritten then)
            seg_host = both[:-1]
        rows = int(seg_host[-1])
        src = torch.empty(rows, dtype=torch.int32, device=dev)
        _lib.check(lib.hnrf_segment_scatter(_ptr(member), _ptr(weight_rec), float(weight_min), total, P, _ptr(status),
                                            ws.data_ptr(), ws.numel() * 4, _ptr(src), rows, _stream()),
                   'hnrf_segment_scatter')
    return seg_host, src


# -------------------------------------------------------------------------------------------------- geometry maps
def ray_surface(near, far, alpha, depth, weights=None, offsets=None, alpha_min=0.5, want_median=False, want_woff=False,
                out=None):
    """hnrf_ray_surface (include/hnrf_geometry.h): near, far, alpha, depth (R,), weights (R, S) and offsets (R, S, 3) or
    None (lean) -> {'t_exp' (R,), 'valid' (R,) uint8, and when asked for 't_med' (R,), 'woff' (R, 3)}.  ``out``: a dict
    of tensors to write into (a per-frame workspace)."""
    lib = _lib.load_geometry()
    _chk(near, far, alpha, depth, weights, offsets)
    R = alpha.shape[0]
    S = int(weights.shape[1]) if weights is not None else 1
    if any(v.shape != (R,) for v in (near, far, alpha, depth)) or (weights is not None and weights.shape != (R, S)) or \
            (offsets is not None and (weights is None or offsets.shape != (R, S, 3))):
        raise _lib.HnrfError('ray_surface: near, far, alpha, depth (R,), weights (R, S), offsets (R, S, 3) expected')
    dev = alpha.device
    out = {} if out is None else out
    res = {'t_exp': out.get('t_exp'), 'valid': out.get('valid'), 't_med': out.get('t_med') if want_median else None,
           'woff': out.get('woff') if want_woff else None}
    if res['t_exp'] is None:
        res['t_exp'] = torch.empty(R, device=dev)
    if res['valid'] is None:
        res['valid'] = torch.empty(R, dtype=torch.uint8, device=dev)
    if want_median and res['t_med'] is None:
        res['t_med'] = torch.empty(R, device=dev)
    if want_woff and res['woff'] is None:
        res['woff'] = torch.empty(R, 3, device=dev)
    _chk(res['t_exp'], res['t_med'], res['woff'])
    _chk_dev(res['valid'], torch.uint8, 'ray_surface: valid')
    if res['t_exp'].numel() < R or res['valid'].numel() < R or (want_median and res['t_med'].numel() < R) or \
            (want_woff and res['woff'].numel() < 3 * R):
        raise _lib.HnrfError('ray_surface: an output is smaller than %d rays' % R)
    with torch.cuda.device(dev):
        _lib.check(lib.hnrf_ray_surface(_ptr(near), _ptr(far), _ptr(alpha), _ptr(depth), _ptr(weights), _ptr(offsets), R, S,
                                        float(alpha_min), _ptr(res['t_exp']), _ptr(res['t_med']), _ptr(res['woff']),
                                        _ptr(res['valid']), _stream()), 'hnrf_ray_surface')
    return {k: v for k, v in res.items() if v is not None}


def pixel_rays(ray_index, H, W, pix2ray=None, status=None):
    """hnrf_pixel_rays: ray_index (N,) int64 -> pix2ray (H * W,) int32 and status (1,) int32, both device tensors; the
    status is not read back here."""
    lib = _lib.load_geometry()
    _chk_dev(ray_index, torch.int64, 'pixel_rays: ray_index')
    H, W, dev = int(H), int(W), ray_index.device
    pix2ray = torch.empty(max(H * W, 0), dtype=torch.int32, device=dev) if pix2ray is None else pix2ray
    status = torch.zeros(1, dtype=torch.int32, device=dev) if status is None else status
    _chk_dev(pix2ray, torch.int32, 'pixel_rays: pix2ray')
    _chk_dev(status, torch.int32, 'pixel_rays: status')
    if ray_index.dim() != 1 or pix2ray.numel() < H * W or status.numel() < 1:
        raise _lib.HnrfError('pixel_rays: ray_index (N,) and pix2ray of H * W = %d elements expected' % (H * W))
    with torch.cuda.device(dev):
        _lib.check(lib.hnrf_pixel_rays(_ptr(ray_index), ray_index.numel(), H, W, _ptr(pix2ray), _ptr(status), _stream()),
                   'hnrf_pixel_rays')
    return pix2ray, status


GEOMETRY_OUTPUTS = ('normal', 'nvalid', 'normal8', 'depth8', 'shaded8', 'offset8')


def geometry_maps(rays_o, rays_d, surf, pix2ray, H, W, want, surface=0, alpha=None, edge=0.05, M=None, bgcolor=None,
                  lohi=None, ambient=0.25, albedo=0.8, truth8=None, status=None, out=None):
    """hnrf_geometry_maps: ``surf`` = what ray_surface returned, ``want`` = names out of GEOMETRY_OUTPUTS -> {name:
    tensor}: normal (H, W, 3) fp32, nvalid (H, W) uint8, the 8-bit panels (H, W, 3) uint8.  ``out``: tensors to write
    into."""
    lib = _lib.load_geometry()
    bad = [k for k in want if k not in GEOMETRY_OUTPUTS]
    if bad:
        raise _lib.HnrfError('geometry_maps: unknown outputs %r (out of %r)' % (bad, GEOMETRY_OUTPUTS))
    _chk(rays_o, rays_d, alpha, M, bgcolor, lohi, surf.get('t_exp'), surf.get('t_med'), surf.get('woff'))
    _chk_dev(pix2ray, torch.int32, 'geometry_maps: pix2ray')
    _chk_dev(surf['valid'], torch.uint8, 'geometry_maps: valid')
    H, W, N, dev = int(H), int(W), rays_o.shape[0], rays_o.device
    if rays_o.shape != (N, 3) or rays_d.shape != (N, 3) or pix2ray.numel() < H * W or surf['valid'].numel() < N or \
            any(v is not None and v.numel() < N * k for v, k in ((surf.get('t_exp'), 1), (surf.get('t_med'), 1),
                                                                   (surf.get('woff'), 3), (alpha, 1))):
        raise _lib.HnrfError('geometry_maps: rays (N, 3), per-ray inputs of N = %d rays and pix2ray of H * W expected' % N)
    for name, v, k in (('M', M, 9), ('bgcolor', bgcolor, 3), ('lohi', lohi, 2)):
        if v is not None and v.numel() != k:
            raise _lib.HnrfError('geometry_maps: %s must hold %d floats' % (name, k))
    if truth8 is not None:
        _chk_dev(truth8, torch.uint8, 'geometry_maps: truth8')
        if truth8.numel() != H * W * 3:
            raise _lib.HnrfError('geometry_maps: truth8 must be (H, W, 3)')
    if status is not None:
        _chk_dev(status, torch.int32, 'geometry_maps: status')
    out = {} if out is None else out
    res = {}
    for k in want:
        shape, dtype = ((H, W, 3), torch.float32) if k == 'normal' else ((H, W), torch.uint8) if k == 'nvalid' else \
            ((H, W, 3), torch.uint8)
        t = out.get(k)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        _chk_dev(t, dtype, 'geometry_maps: ' + k)
        if tuple(t.shape) != shape:
            raise _lib.HnrfError('geometry_maps: %s must be %r, got %r' % (k, shape, tuple(t.shape)))
        res[k] = t
    with torch.cuda.device(dev):
        _lib.check(lib.hnrf_geometry_maps(_ptr(rays_o), _ptr(rays_d), _ptr(surf.get('t_exp')), _ptr(surf.get('t_med')),
                                          _ptr(surf['valid']), int(surface), _ptr(alpha), _ptr(surf.get('woff')),
                                          _ptr(pix2ray), N, H, W, float(edge), _ptr(M), _ptr(bgcolor), _ptr(lohi),
                                          float(ambient), float(albedo), _ptr(truth8), _ptr(status),
                                          *[_ptr(res.get(k)) for k in GEOMETRY_OUTPUTS], _stream()), 'hnrf_geometry_maps')
    return res


# ------------------------------------------------------------------------------------------ density-gradient normals
GRADIENT_CHUNK = 16384
# bytes of workspace per sample of a chunk, 'f32' and 'f16x3' alike (both save fp32 activations):
#   canonical  raw 16 + pe 252 + acts 8192 + relu_bits 256 + d_raw 16 + dZ 8192
#   non-rigid  xyz 12 + offsets 12 + pe 144 + acts 3072 + relu_bits 96 + dZ 3072
GRADIENT_BYTES_CANONICAL, GRADIENT_BYTES_NONRIGID = 16924, 6408


def _gradient_workspace(ws, C, with_warp, dev):
    key = (int(C), str(dev))
    if ws.get('key') != key:
        ws.clear()
        ws['key'] = key
        d_raw = torch.zeros(C, 4, device=dev)
        d_raw[:, 3] = 1.0
        names = ('raw', 'pe', 'acts', 'bits', 'dZ')
        ws.update(zip(names, _train_buffers('canonical', names, C, 'f32', dev, lead=(C,))), d_raw=d_raw,
                  one=torch.ones(1, device=dev), amax=torch.zeros(1, device=dev))
    if with_warp and 'nr_acts' not in ws:
        names = ('xyz', 'offsets', 'pe', 'acts', 'bits', 'dZ')
        ws.update(zip(('nr_xyz', 'nr_off', 'nr_pe', 'nr_acts', 'nr_bits', 'nr_dZ'),
                      _train_buffers('nonrigid', names, C, 'f32', dev, lead=(C,))))
    return ws


def density_gradient(xyz, cnl_packed, cnl_weights, mode='f32', warp=None, workspace=None, chunk=GRADIENT_CHUNK):
    """The gradient of the canonical MLP's density with respect to position, by the training kernels: g (P, 3) fp32 and
    sigma (P,) (the pre-activation density, raw[:, 3]).

    ``xyz`` (P, 3): canonical points; ``cnl_packed``: the forward image (canonical_pack) of ``mode`` ('f32' | 'f16x3');
    ``cnl_weights``: the backward image (canonical_bwd_pack: one tensor, what a caller keeps) or the 9 nn.Linear
    weights, packed here then.  The forward is hnrf_canonical_fwd_train, the backward hnrf_canonical_bwd with
    d_raw = (0, 0, 0, 1) in every row and d_raw_amax = 1, a resident one-element tensor.

    ``warp`` = (x_skel (P, 3), hann_w (6,), nr_packed, nr_weights (the backward image or the 7 weights)): the points are
    skeleton-space points, xyz = hnrf_nonrigid_fwd_train(x_skel) (``xyz`` is ignored: pass None) and the result is
    hnrf_nonrigid_bwd's d_x_skel = d_xyz + J_offset^T d_xyz, with d_xyz_amax the maximum magnitude of d_xyz over ALL P
    samples, reduced on the device and never read back.  For that the pass has two phases: the canonical gradients of
    every chunk first, the non-rigid chain of every chunk behind them (its forward runs a second time for the sign
    masks) -- so that the result does not depend on ``chunk``, bit for bit, in 'f16x3' too.

    The MLP kernels write activations and per-layer gradients nobody wants here, so the pass runs over at most ``chunk``
    samples at a time through ``workspace``, a dict the caller keeps (filled here; {} or None = a fresh one).  It takes
    GRADIENT_BYTES_CANONICAL = 16924 bytes per sample of a chunk in either mode, and GRADIENT_BYTES_NONRIGID = 6408 more
    with ``warp`` (277 MB and 382 MB at the default chunk of 16384).  Nothing synchronises."""
    if mode not in MLP_MODES:
        raise _lib.HnrfError("density_gradient: mode must be 'f32' or 'f16x3', got %r" % (mode,))
    C = int(chunk)
    if C < 1:
        raise _lib.HnrfError('density_gradient: chunk must be >= 1, got %r' % (chunk,))
    if warp is not None:
        x_skel, hann_w, nr_packed, nr_weights = warp
        _chk(x_skel, hann_w, nr_packed)
        x_skel = x_skel.reshape(-1, 3)
        P, dev = x_skel.shape[0], x_skel.device
    else:
        _chk(xyz)
        xyz = xyz.reshape(-1, 3)
        P, dev = xyz.shape[0], xyz.device
    _chk(cnl_packed)
    g, sigma = torch.empty(P, 3, device=dev), torch.empty(P, device=dev)
    if P == 0:
        return g, sigma
    if not torch.is_tensor(cnl_weights):
        cnl_weights = canonical_bwd_pack(list(cnl_weights), mode)
    _chk(cnl_weights)
    if warp is not None:
        if not torch.is_tensor(nr_weights):
            nr_weights = nonrigid_bwd_pack(list(nr_weights), mode)
        _chk(nr_weights)
    ws = _gradient_workspace({} if workspace is None else workspace, min(C, max(P, 1)) if workspace is None else C,
                             warp is not None, dev)
    C = ws['key'][0]
    # the chunks' saved buffers are the workspace's (a last, shorter chunk uses their front: hence P = n)
    if warp is not None:
        nr_out = {'xyz': ws['nr_xyz'], 'offsets': ws['nr_off'], 'pe': ws['nr_pe'], 'acts': ws['nr_acts'], 'bits': ws['nr_bits']}
    with torch.cuda.device(dev):
        for i in range(0, P, C):
            n = min(C, P - i)
            if warp is not None:
                nonrigid_train(x_skel[i:i + n], hann_w, nr_packed, mode, out=nr_out)
                pts = ws['nr_xyz']
            else:
                pts = xyz[i:i + n]
            canonical_train(pts, cnl_packed, mode, out=ws, P=n)
            canonical_bwd(pts, ws['d_raw'], ws['bits'], cnl_weights, mode, out={'dZ': ws['dZ'], 'd_xyz': g[i:i + n], 'amax': None},
                          d_raw_amax=ws['one'], P=n)
            sigma[i:i + n].copy_(ws['raw'][:n, 3])
        if warp is not None:
            d_xyz = g.clone()
            torch.amax(d_xyz.abs().reshape(-1), dim=0, keepdim=True, out=ws['amax'])
            for i in range(0, P, C):
                n = min(C, P - i)
                nonrigid_train(x_skel[i:i + n], hann_w, nr_packed, mode, out=nr_out)
                nonrigid_bwd(x_skel[i:i + n], hann_w, d_xyz[i:i + n], ws['nr_bits'], nr_weights, mode,
                             out={'dZ': ws['nr_dZ'], 'd_x_skel': g[i:i + n], 'amax': None}, d_xyz_amax=ws['amax'], P=n)
    return g, sigma


def ray_normals(weights, bmw, motion_Rs, idx, count, g, alpha, alpha_min=0.5, workspace=None, out=None):
    """hnrf_ray_normals (include/hnrf_normals.h): weights (R, S), bmw (R, S, B), motion_Rs (B, 3, 3), idx / count from
    compact_samples(weights, weight_min), g (n, 3) the gradient at the first n kept samples, alpha (R,) -> (normal (R, 3),
    nvalid (R,) uint8).  ``workspace``: an int32 tensor of R S elements, 256-byte aligned, to use as the slot table (one
    that is too small or misaligned is replaced by a fresh one); ``out``: (normal, nvalid) to write into."""
    lib = _lib.load_normals()
    _chk(weights, bmw, motion_Rs, g, alpha)
    _chk_dev(idx, torch.int32, 'ray_normals: idx')
    _chk_dev(count, torch.int32, 'ray_normals: count')
    if weights.dim() != 2 or bmw.dim() != 3 or bmw.shape[:2] != weights.shape or motion_Rs.shape != (bmw.shape[2], 3, 3) \
            or g.dim() != 2 or g.shape[1] != 3 or alpha.shape != (weights.shape[0],):
        raise _lib.HnrfError('ray_normals: weights (R, S), bmw (R, S, B), motion_Rs (B, 3, 3), g (n, 3), alpha (R,) '
                             'expected, got %s %s %s %s %s' % (tuple(weights.shape), tuple(bmw.shape),
                                                               tuple(motion_Rs.shape), tuple(g.shape), tuple(alpha.shape)))
    R, S = weights.shape
    dev = weights.device
    n_max = min(int(g.shape[0]), int(idx.numel()))
    need = lib.hnrf_ray_normals_workspace_bytes(R, S)
    if workspace is None or workspace.numel() * 4 < need or workspace.data_ptr() % 256:      # (a slice may be misaligned)
        workspace = torch.empty(max((need + 3) // 4, 1), dtype=torch.int32, device=dev)
    _chk_dev(workspace, torch.int32, 'ray_normals: workspace')
    normal, nvalid = out if out is not None else (torch.empty(R, 3, device=dev), torch.empty(R, dtype=torch.uint8, device=dev))
    _chk(normal)
    _chk_dev(nvalid, torch.uint8, 'ray_normals: nvalid')
    if normal.numel() < 3 * R or nvalid.numel() < R:
        raise _lib.HnrfError('ray_normals: an output is smaller than %d rays' % R)
    with torch.cuda.device(dev):
        _lib.check(lib.hnrf_ray_normals(_ptr(weights), _ptr(bmw), _ptr(motion_Rs), _ptr(idx), _ptr(count), n_max, _ptr(g),
                                        _ptr(alpha), R, S, int(bmw.shape[2]), float(alpha_min), _ptr(workspace),
                                        workspace.numel() * 4, _ptr(normal), _ptr(nvalid), _stream()), 'hnrf_ray_normals')
    return normal, nvalid


NORMAL_OUTPUTS = ('normal', 'nvalid', 'normal8', 'shaded8')


def normal_panels(rays_d, ray_normal, ray_nvalid, valid, pix2ray, H, W, want, surface=0, alpha=None, M=None, bgcolor=None,
                  ambient=0.25, albedo=0.8, status=None, out=None):
    """hnrf_normal_panels: per-ray normals (ray_normals), ``valid`` of ray_surface and pix2ray of pixel_rays -> {name:
    tensor} for ``want`` out of NORMAL_OUTPUTS: normal (H, W, 3) fp32, nvalid (H, W) uint8, normal8 / shaded8 (H, W, 3)
    uint8.  ``out``: tensors to write into."""
    lib = _lib.load_normals()
    bad = [k for k in want if k not in NORMAL_OUTPUTS]
    if bad:
        raise _lib.HnrfError('normal_panels: unknown outputs %r (out of %r)' % (bad, NORMAL_OUTPUTS))
    _chk(rays_d, ray_normal, alpha, M, bgcolor)
    _chk_dev(pix2ray, torch.int32, 'normal_panels: pix2ray')
    _chk_dev(ray_nvalid, torch.uint8, 'normal_panels: ray_nvalid')
    _chk_dev(valid, torch.uint8, 'normal_panels: valid')
    H, W, N, dev = int(H), int(W), rays_d.shape[0], rays_d.device
    if rays_d.shape != (N, 3) or pix2ray.numel() < H * W or ray_normal.numel() < 3 * N or ray_nvalid.numel() < N or \
            valid.numel() < N or (alpha is not None and alpha.numel() < N):
        raise _lib.HnrfError('normal_panels: rays_d (N, 3), per-ray inputs of N = %d rays and pix2ray of H * W expected' % N)
    for name, v, k in (('M', M, 9), ('bgcolor', bgcolor, 3)):
        if v is not None and v.numel() != k:
            raise _lib.HnrfError('normal_panels: %s must hold %d floats' % (name, k))
    if status is not None:
        _chk_dev(status, torch.int32, 'normal_panels: status')
    out = {} if out is None else out
    res = {}
    for k in want:
        shape, dtype = ((H, W, 3), torch.float32) if k == 'normal' else ((H, W), torch.uint8) if k == 'nvalid' else \
            ((H, W, 3), torch.uint8)
        t = out.get(k)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        _chk_dev(t, dtype, 'normal_panels: ' + k)
        if tuple(t.shape) != shape:
            raise _lib.HnrfError('normal_panels: %s must be %r, got %r' % (k, shape, tuple(t.shape)))
        res[k] = t
    with torch.cuda.device(dev):
        _lib.check(lib.hnrf_normal_panels(_ptr(rays_d), _ptr(ray_normal), _ptr(ray_nvalid), _ptr(valid), int(surface),
                                          _ptr(alpha), _ptr(pix2ray), N, H, W, _ptr(M), _ptr(bgcolor), float(ambient),
                                          float(albedo), _ptr(status), *[_ptr(res.get(k)) for k in NORMAL_OUTPUTS],
                                          _stream()), 'hnrf_normal_panels')
    return res


def field_normals(verts, g, sigma, vol, n_bones, bbox_min, bbox_scale):
    """hnrf_field_normals: verts (V, 3) canonical, g (V, 3) and sigma (V,) of density_gradient there, vol (>= n_bones,
    G, G, G) -> normal (V, 3): -grad D / |grad D| of D = relu(sigma) fg, 0 where the length is 0 or not finite."""
    lib = _lib.load_normals()
    _chk(verts, g, sigma, vol, bbox_min, bbox_scale)
    V, G = verts.shape[0], vol.shape[-1]
    if verts.shape != (V, 3) or g.shape != (V, 3) or sigma.shape != (V,) or vol.dim() != 4 or vol.shape[0] < n_bones or \
            vol.shape[1] != G or vol.shape[2] != G or bbox_min.numel() != 3 or bbox_scale.numel() != 3:
        raise _lib.HnrfError('field_normals: verts (V, 3), g (V, 3), sigma (V,), vol (>= B, G, G, G), bbox_min / '
                             'bbox_scale (3,) expected')
    normal = torch.empty(V, 3, device=verts.device)
    with torch.cuda.device(verts.device):
        _lib.check(lib.hnrf_field_normals(_ptr(verts), _ptr(g), _ptr(sigma), V, _ptr(vol), int(n_bones), G, _ptr(bbox_min),
                                          _ptr(bbox_scale), _ptr(normal), _stream()), 'hnrf_field_normals')
    return normal
