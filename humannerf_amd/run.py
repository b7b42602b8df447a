"""The render modes of the reference's run.py as functions over this package's pieces (the
callers on the far side of the path).  No command line: the reference's own run.py keeps working unchanged with
``network_module: 'humannerf_amd.network'``; these are for callers that want the whole loop on
the MI355X-native side -- dataset.Subject frames (camera only: rays are generated on the device), render.render_frames
(frame-sharded over the ranks, images unpacked and quantised on the device, asynchronous copies to pinned memory),
render.ImageWriter / MetricsWriter on worker threads.

  run_movement   run.py:212-445   every frame of the subject with its own camera and pose; render | truth (| alpha)
                                  side by side, PSNR (SSIM, LPIPS) per image and averaged
  run_freeview   run.py:67-170    one training frame seen from a camera orbiting the subject
  run_tpose      run.py:178-183   the canonical pose on a turntable, non-rigid motion off
  run_heads      run.py:76-81, 219-225   the three loops above for a multi-head canonical MLP with cfg.test.head_id = -1:
                                  every frame rendered once, head i written to ``<load_net><tag>_h<i>/<folder>``
  run_mesh       (no counterpart) the canonical body as a coloured triangle mesh, and that mesh skinned into frames
  run_gltf       (no counterpart) that mesh, its skeleton, its 4 or 8 largest bone weights per vertex and the movement as
                                  ONE animated glTF 2.0 binary, with the skinning error of the truncation per frame
  run_mesh_render (no counterpart) the movement / freeview / tpose sequences as rasterised pictures of that mesh: a preview
  run_surface_points  run.py:388-404   cfg.test.save_3d_together: one canonical surface point per ray of every movement
                                  frame, collected as ``name-2-3d.bin``
  run_distance_matrix tools/compute_distance*.py   the frame x frame appearance distance of those records
  run_compare_lbs_delta compare_lbs_delta.py   every movement frame with and without the non-rigid motions, next to the
                                  colour map of the weighted non-rigid offset and the truth, both PSNRs in the file name

cfg.amd.maps (a list out of 'depth', 'normal', 'shaded', 'offset') adds geometry panels to every frame of the loops:
``[render | truth | alpha | maps...]`` in the PNG and in the video (humannerf_amd/geometry.py: screen-space differences of
the rendered surface distance, computed on the device in the frame's launches).

Output layout as in the reference: ``<logdir>/<load_net><eval_output_tag>/<folder>/NAME.png`` plus
``<folder>-metrics.perimg.txt / .average.txt`` (movement) and the stacked frames (MP4 when imageio is importable).
cfg.amd.video = 'mjpeg' adds ``<folder>.avi`` (Motion-JPEG of the same panels, encoded on the device; the result dict's
``'video'``), 'mjpeg_only' writes that file and no PNG; with world > 1 ``<folder>.rank<r>.avi`` per rank, joined by
video.merge_parts.
With world > 1 every rank writes its own frames into the same folder; metrics are reduced by the caller
(``MetricsWriter`` files are per rank: ``<folder>.rank<r>``).
"""
import contextlib
import os

import numpy as np

from . import render
from .config import cfg


def _output_dir(logdir=None):
    return os.path.join(logdir if logdir is not None else cfg.get('logdir', '.'),
                        str(cfg.get('load_net', 'latest')) + str(cfg.get('eval_output_tag', '')))


class _Frames:
    """Sequence of per-frame input dicts built on demand (a movement sequence holds an image per frame)."""

    def __init__(self, n, make):
        self.n, self.make = n, make

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.make(i)


def _sequence(subject, kind, load_image=True, device=None, test_num=-1, frame_idx=None, total_frames=None,
              image_size=None, src_type='zju_mocap', numbered=False, square_tpose=False, prefix=''):
    """(frames, names, default folder) of the ``kind`` = 'movement' | 'freeview' | 'tpose' sequence, for every loop below.
    movement: the subject's first ``test_num`` frames (< 0: all) under their frame names, with their images (truth panel
    and metrics; decoded for ``device``) or -- ``load_image`` False -- camera only at ``image_size`` / the image's own size.
    freeview (freeview.py:172-280) and tpose (tpose.py): ``total_frames`` cameras (None: cfg.render_frames) on
    cfg.bgcolor, like every non-train dataset the reference builds (create_dataset.py:40); names None, ``numbered``
    '%06d'; ``src_type`` None: not handed on; ``square_tpose``: the T-pose camera gets the larger side of ``image_size``.
    Default folder: ``prefix`` + movement / freeview_<frame_idx> / tpose; without a prefix cfg.render_folder_name goes
    before the latter two."""
    if kind == 'movement':
        n = len(subject) if test_num < 0 else min(test_num, len(subject))
        if load_image:
            # camera-only rays: they come from the device generator, the truth pixels are picked on the device (the
            # prefetcher thread of render_frames builds them: PNG decoding on the host, undistortion / composite / resize
            # on the device when there is one)
            make = lambda i: subject.movement_frame(i, load_image=True, device=device)
        else:
            size = lambda i: image_size if image_size is not None else subject.image_size(subject.framelist[i])
            make = lambda i: subject.movement_frame(i, image_size=size(i))
        return _Frames(n, make), [str(subject.framelist[i]).replace('/', '-') for i in range(n)], prefix + 'movement'
    n = int(cfg.get('render_frames', 100)) if total_frames is None else int(total_frames)
    if kind == 'freeview':
        frame_idx = int(cfg.get('freeview', {}).get('frame_idx', 0)) if frame_idx is None else int(frame_idx)
        if image_size is None:
            image_size = subject.image_size(subject.framelist_all[frame_idx])
        src = {} if src_type is None else {'src_type': src_type}
        make = lambda i: subject.freeview_frame(i, n, train_frame_idx=frame_idx, image_size=image_size,
                                                bgcolor=cfg.bgcolor, **src)
        folder = 'freeview_%d' % frame_idx
    else:
        size = int(np.max(image_size)) if square_tpose and image_size is not None else image_size
        make = lambda i: subject.tpose_frame(i, n, image_size=size, bgcolor=cfg.bgcolor)
        folder = 'tpose'
    folder = prefix + folder if prefix else cfg.get('render_folder_name', '') or folder
    return _Frames(n, make), ['%06d' % i for i in range(n)] if numbered else [None] * n, folder


_CFG_KEYS = ('perturb', 'ignore_non_rigid_motions', 'show_truth')


@contextlib.contextmanager
def _cfg_override(**values):
    """cfg.perturb, cfg.ignore_non_rigid_motions, cfg.show_truth and ``diagnostics`` (cfg.amd['diagnostics']) set for the
    block and put back behind it, an exception included.  An amd key that was not there is popped again (show_truth comes
    back as False); without an amd node ``diagnostics`` does nothing."""
    amd = cfg.get('amd', None)
    if 'diagnostics' in values and amd is None:
        del values['diagnostics']
    assert set(values) <= set(_CFG_KEYS + ('diagnostics',)), sorted(values)
    had_diag = 'diagnostics' in values and 'diagnostics' in amd
    old = {k: amd.get(k) if k == 'diagnostics' else cfg.get(k, False) for k in values}
    try:
        for k, v in values.items():
            if k == 'diagnostics':
                amd[k] = v
            else:
                setattr(cfg, k, v)
        yield
    finally:
        for k, v in old.items():
            if k != 'diagnostics':
                setattr(cfg, k, v)
            elif had_diag:
                amd[k] = v
            else:
                amd.pop(k, None)


def _panels(rgb8, alpha8, truth8=None):
    """run.py:143-149 / 359-364: [render | truth if cfg.show_truth | alpha if cfg.show_alpha]."""
    return np.concatenate(render.select_panels(rgb8, alpha8, truth8), axis=1)


class _VideoOut:
    """cfg.amd.video of a render loop: the device encoder to hand to the loop (``encoder``, None for 'none'), the
    collector of its streams (``add(i, bytes)``) and the file at the end (``finalize() -> path or None``):
    ``<image_dir>.avi``, ``<image_dir>.rank<r>.avi`` with world > 1 (video.merge_parts joins the ranks' files).  A frame
    without a name is called by its index, %06d, like ImageWriter calls it."""

    def __init__(self, image_dir, names, rank, world, device):
        from . import video
        from .config import amd_option, check_amd_options
        check_amd_options()
        self.mode = amd_option('video', 'none')
        self.only = self.mode == 'mjpeg_only'
        self.encoder = self.writer = None
        self.names = names
        if self.mode == 'none':
            return
        self._video = video
        self.fps = int(amd_option('video_fps', 10))
        self.encoder = video.JpegEncoder(device, int(amd_option('video_quality', 90)))
        self.path = image_dir.rstrip('/') + ('.avi' if world == 1 else '.rank%d.avi' % rank)

    def add(self, i, data):
        if self.writer is None:
            height, width = self._video.jpeg_size(data)
            self.writer = self._video.MjpegWriter(self.path, width, height, self.fps)
        self.writer.add(self.names[i] if self.names[i] is not None else '%06d' % i, data)

    def finalize(self):
        return self.writer.finalize() if self.writer is not None else None


def _baked_folder(network, subject, folder):
    """cfg.amd.canonical = 'baked': bake the canonical grid over the subject's canonical bbox before the first frame
    (so that no frame of the loop pays for it) and mark the folder ``<folder>_baked_<N>`` -- ``<folder>_baked_<N>_nr<M>``
    with cfg.amd.nonrigid = 'baked' where the non-rigid motions are on -- : approximate pictures are never written where
    exact ones go.  An injected grid (Network.set_baked_grid) is used as it is."""
    from .config import amd_option, check_amd_options
    _, nonrigid, nr_M = check_amd_options()
    if amd_option('canonical', 'mlp') != 'baked':
        return folder
    bbox = subject.canonical_bbox
    mn, mx = bbox['min_xyz'].astype('float32'), bbox['max_xyz'].astype('float32')
    import torch
    with torch.no_grad():
        network._baked_for_frame(torch.from_numpy(mn), torch.from_numpy(mx), None)    # (an injected grid: returned as it is)
    folder = '%s_baked_%d' % (folder, network.baked_resolution)
    if nonrigid == 'baked' and not cfg.ignore_non_rigid_motions:
        folder += '_nr%d' % nr_M                # the per-frame offset grid (cfg.amd.nonrigid = 'baked'): baked by forward
    return folder


def _render_loop(network, frames, names, folder, logdir, rank, world, device, metrics=None, on_device=False,
                 lpips_fn=None):
    """``metrics``: a MetricsWriter.  ``on_device``: its values come from render_frames' device pass (cfg.amd.metrics =
    'device') instead of MetricsWriter.append on the delivered images."""
    out_dir = _output_dir(logdir)
    device = device or next(network.parameters()).device
    vout = _VideoOut(os.path.join(out_dir, folder), names, rank, world, device)
    writer = None if vout.only else render.ImageWriter(out_dir, folder)          # 'mjpeg_only': no PNG, no directory
    own = list(range(rank, len(frames), world))

    from .config import amd_option
    maps = list(amd_option('maps', []) or [])
    held = {}                                       # with maps: a frame's images between on_image and its on_maps

    def on_image(i, rgb8, alpha8, truth8=None):
        if maps:
            held[i] = (rgb8, alpha8, truth8)
        else:
            writer.append(_panels(rgb8, alpha8, truth8), img_name=names[i])
        if metrics is not None and truth8 is not None and not on_device:
            metrics.append(name=names[i], pred=rgb8, target=truth8, mask=None)

    def on_maps(i, panels):
        writer.append(np.concatenate(render.select_panels(*held.pop(i), maps=panels), axis=1), img_name=names[i])

    extra = {}
    if maps:
        extra = dict(maps=maps, on_maps=on_maps)
    if vout.encoder is not None:
        extra.update(video=vout.encoder, on_video=vout.add, images='none' if vout.only else 'host')
    if metrics is not None and on_device:
        extra.update(metrics=metrics.metrics, lpips_fn=lpips_fn,
                     on_metrics=lambda i, values: metrics.append_values(names[i], values))
    with _cfg_override(perturb=0.):                                    # run.py:71, 214 (render_frames zeroes it as well)
        images = render.render_frames(network, frames, rank=rank, world=world, device=device, on_image=on_image,
                                      show_truth=True, **extra)
    stack = writer.finalize() if writer is not None else None
    averages = metrics.finalize() if metrics is not None else None
    result = {'frames': own, 'images': images, 'image_dir': os.path.join(out_dir, folder), 'stack': stack,
              'metrics': averages}
    if vout.encoder is not None:
        result['video'] = vout.finalize()
    return result


def run_movement(network, subject, render_folder_name='movement', logdir=None, rank=0, world=1, device=None,
                 test_num=-1, metrics=None, lpips_fn=None):
    """run.py:212-445.  Frames are loaded with their images (truth panel and metrics), rays come from the device ray
    generator.  Returns the per-rank result dict of the loop; ``['metrics']`` holds this rank's averages.
    cfg.amd.metrics = 'device' computes them in the frame's launches on the GPU (render.render_frames(metrics=...)) and
    writes the same files; on a CPU device it raises."""
    from .config import amd_option, check_amd_options
    check_amd_options()
    device = device or next(network.parameters()).device
    on_device = amd_option('metrics', 'host') == 'device'
    if on_device and device.type != 'cuda':
        raise ValueError("cfg.amd.metrics = 'device' needs a GPU, got device %s" % device)
    cfg.show_truth = True                       # lasting, not an override: the reference's run.py:216 leaves it set too
    frames, names, _ = _sequence(subject, 'movement', device=device, test_num=test_num)
    render_folder_name = _baked_folder(network, subject, render_folder_name)
    suffix = '' if world == 1 else '.rank%d' % rank
    mw = render.MetricsWriter(_output_dir(logdir), render_folder_name + suffix, dataset=subject.dataset_path,
                              metrics=metrics, lpips_fn=lpips_fn)
    return _render_loop(network, frames, names, render_folder_name, logdir, rank, world, device, metrics=mw,
                        on_device=on_device, lpips_fn=lpips_fn)


def run_freeview(network, subject, frame_idx=None, total_frames=None, render_folder_name=None, logdir=None, rank=0,
                 world=1, device=None, image_size=None, src_type='zju_mocap'):
    """run.py:67-176 with data_type 'freeview' (freeview.py:172-280)."""
    # numbered: with world > 1 the frames are named %06d, else None (ImageWriter then numbers what it is given)
    frames, names, folder = _sequence(subject, 'freeview', frame_idx=frame_idx, total_frames=total_frames,
                                      image_size=image_size, src_type=src_type, numbered=world > 1)
    folder = _baked_folder(network, subject, render_folder_name or folder)
    return _render_loop(network, frames, names, folder, logdir, rank, world, device)


def run_tpose(network, subject, total_frames=None, render_folder_name=None, logdir=None, rank=0, world=1, device=None,
              image_size=None):
    """run.py:178-183: the turntable of tpose.py with cfg.ignore_non_rigid_motions = True."""
    # numbered: with world > 1 the frames are named %06d, else None (as in run_freeview)
    frames, names, folder = _sequence(subject, 'tpose', total_frames=total_frames, image_size=image_size,
                                      numbered=world > 1)
    with _cfg_override(ignore_non_rigid_motions=True):
        folder = _baked_folder(network, subject, render_folder_name or folder)
        return _render_loop(network, frames, names, folder, logdir, rank, world, device)


def run_heads(network, subject, kind='movement', frame_idx=None, total_frames=None, render_folder_name=None, logdir=None,
              device=None, test_num=-1, metrics=None, lpips_fn=None, image_size=None, src_type='zju_mocap'):
    """Every head of a multi-head canonical MLP (run.py:76-81, :219-225 with cfg.test.head_id = -1): each frame of the
    ``kind`` = 'movement' | 'freeview' | 'tpose' sequence is rendered ONCE with ``head_id = -1`` -- the trunks of both
    MLPs once, one compositing pass per head -- and head i's picture goes to ``<logdir>/<load_net><eval_output_tag>_h<i>/
    <folder>/NAME.png``, as the reference names them; 'movement' also writes ``<folder>-metrics.perimg.txt /
    .average.txt`` per head (MetricsWriter on the delivered images).  Frames leave through render.FrameOutbox and
    render.ImageWriter like those of the other loops.  The f16-range verdict of a frame is waited for before its pictures
    are handed over (one wait per frame; with cfg.amd.on_f16_range = 'f32' a frame out of range is rendered again with
    the exact kernels first).  Returns a list of per-head result dicts {'image_dir', 'stack', 'metrics'}.
    cfg.amd.video and cfg.amd.maps are not built for this loop: ValueError."""
    import torch
    from .config import amd_option, check_amd_options
    check_amd_options()
    if amd_option('video', 'none') != 'none':
        raise ValueError("run_heads: cfg.amd.video = %r is not built for the all-heads loop (set it to 'none')"
                         % (amd_option('video', 'none'),))
    if amd_option('maps', []):
        raise ValueError('run_heads: cfg.amd.maps = %r is not built for the all-heads loop (set it to [])'
                         % (list(amd_option('maps', [])),))
    H = getattr(network, 'head_num', 0)
    if not H:
        raise ValueError('run_heads: the canonical MLP has a single head (canonical_mlp.multihead.enable is off)')
    if kind not in ('movement', 'freeview', 'tpose'):
        raise ValueError("run_heads: kind must be 'movement', 'freeview' or 'tpose', got %r" % (kind,))
    device = device or next(network.parameters()).device
    frames, names, folder = _sequence(subject, kind, device=device, test_num=test_num, frame_idx=frame_idx,
                                      total_frames=total_frames, image_size=image_size, src_type=src_type)
    folder, n = render_folder_name or folder, len(frames)
    # perturb: run.py:71, 214.  All three are put back behind the loop whatever the kind sets -- show_truth too, unlike
    # run_movement's, and as False where cfg had none
    override = dict(perturb=0., show_truth=kind == 'movement' or cfg.get('show_truth', False),
                    ignore_non_rigid_motions=kind == 'tpose' or cfg.ignore_non_rigid_motions)
    out_dirs = [_output_dir(logdir) + '_h%d' % h for h in range(H)]
    writers = [render.ImageWriter(d, folder) for d in out_dirs]
    mws = [render.MetricsWriter(d, folder, dataset=subject.dataset_path, metrics=metrics, lpips_fn=lpips_fn)
           for d in out_dirs] if kind == 'movement' else None
    outbox = render.FrameOutbox(device)
    network.eval()

    def render_item(item):
        with torch.no_grad():
            res = network(**item['data'], head_id=-1, iter_val=float(cfg.eval_iter))
        imgs = []
        for h in range(H):
            rgb8, a8, t8 = render.unpack_to_image(item['W'], item['H'], None, item['data']['bgcolor'] / 255., res['rgb'][h],
                                                  res['alpha'][h], item['truth'] if h == 0 else None,
                                                  ray_index=item['ray_index'])
            imgs += [rgb8, a8] + ([t8] if t8 is not None and h == 0 and item['truth'] is not None else [])
        return outbox.post(imgs), item['truth'] is not None

    pre = render.FramePrefetcher(frames, list(range(n)), device, show_truth=kind == 'movement')
    with _cfg_override(**override), contextlib.closing(pre):
        for item in pre:
            mode = network._mlp_mode()
            parcel, has_truth = render_item(item)
            network.check_f16_range(wait=True)                           # (raises, or switches the mode, on a range hit)
            if network._mlp_mode() != mode:
                parcel.discard()
                parcel, has_truth = render_item(item)
            arrs = parcel.collect()[0]
            truth8 = arrs[2] if has_truth else None
            per_head = [arrs[:2]] + [arrs[(3 if has_truth else 2) + 2 * (h - 1):][:2] for h in range(1, H)]
            i = item['idx']
            for h, (rgb8, alpha8) in enumerate(per_head):
                writers[h].append(_panels(rgb8, alpha8, truth8), img_name=names[i])
                if mws is not None and truth8 is not None:
                    mws[h].append(name=names[i], pred=rgb8, target=truth8, mask=None)
    return [{'image_dir': os.path.join(out_dirs[h], folder), 'stack': writers[h].finalize(),
             'metrics': mws[h].finalize() if mws is not None else None} for h in range(H)]


def run_mesh(network, subject, frames=(), resolution=256, level=None, logdir=None, normals=False):
    """Network.extract_canonical_mesh over the subject's canonical bbox, written as ``<out>/mesh/canonical.ply``, and
    for every entry of ``frames`` (index into subject.framelist, or frame name) that mesh posed with
    Network.pose_vertices, written as ``<out>/mesh/<frame_name>.ply`` (vertex colours of the canonical mesh; the
    non-rigid offsets are not inverted).  ``level``: None = Network.MESH_LEVEL.  ``normals``: ``canonical.ply`` also
    holds the density-gradient normals of its vertices (Network.vertex_normals; the posed files do not: a posed normal
    needs the skinning matrix of its vertex).  Returns {name: path}."""
    from . import mesh
    out_dir = os.path.join(_output_dir(logdir), 'mesh')
    os.makedirs(out_dir, exist_ok=True)
    bbox = subject.canonical_bbox
    verts, faces, colors = network.extract_canonical_mesh(
        bbox['min_xyz'], bbox['max_xyz'], subject.motion_weights_priors, resolution=resolution,
        level=network.MESH_LEVEL if level is None else level)
    faces_h, colors_h = faces.cpu().numpy(), colors.cpu().numpy()
    written = {'canonical': os.path.join(out_dir, 'canonical.ply')}
    if normals:
        vn = network.vertex_normals(verts, subject.motion_weights_priors, bbox['min_xyz'], bbox['max_xyz'])
        mesh.write_ply(written['canonical'], verts.cpu().numpy(), faces_h, colors_h, normals=vn.cpu().numpy())
    else:
        mesh.write_ply(written['canonical'], verts.cpu().numpy(), faces_h, colors_h)
    for f in frames:
        idx = subject.framelist.index(f) if isinstance(f, str) else int(f)
        frame = subject.movement_frame(idx, image_size=(1, 1))          # (the camera entries are not used)
        name = str(frame['frame_name']).replace('/', '-')
        written[name] = os.path.join(out_dir, name + '.ply')
        mesh.write_ply(written[name], network.pose_vertices(verts, frame).cpu().numpy(), faces_h, colors_h)
    return written


def run_gltf(network, subject, frames=None, resolution=256, level=None, influences=4, fps=30, up='+z', logdir=None,
             iter_val=1e7, normals=False):
    """The avatar as ONE skinned, animated glTF 2.0 binary, ``<out>/mesh/avatar.glb`` (humannerf_amd/gltf.py): the
    canonical mesh of run_mesh with its vertex colours, the 24-joint skeleton, the ``influences`` (4 or 8) largest bone
    weights of every vertex (Network.skin_weights) and one animation over ``frames`` (indices into subject.framelist or
    frame names; None: the whole framelist; the camera entries are not used) at ``fps``.  ``up``: the up axis of the
    subject's world, '+z' (ZJU-MoCap, the default), '+y' or '-y'.  The pose refiner acts as in Network.pose_vertices
    (``iter_val`` against its kick-in).  The non-rigid offsets are not in the file: skinning cannot represent them.
    ``normals``: the file also holds a NORMAL attribute, the density-gradient normals of the canonical vertices
    (Network.vertex_normals), so that a viewer shades smoothly.

    For every frame the device compares what a viewer will compute, skin.skin_lbs of the truncated weights with the
    frame's joint matrices, with the exact forward skin Network.pose_vertices.  Returns {'path', 'V', 'F', 'frames',
    'kept': {'min', 'mean'} (the sum of the selected weights before normalisation), 'skin_error': {'max', 'mean',
    'per_frame': [{'max', 'mean'}, ...]}} -- distances in metres: the answer to "are 4 influences enough for this
    checkpoint".  Single rank."""
    import torch
    from . import gltf, skin
    out_dir = os.path.join(_output_dir(logdir), 'mesh')
    os.makedirs(out_dir, exist_ok=True)
    bbox = subject.canonical_bbox
    verts, faces, colors = network.extract_canonical_mesh(
        bbox['min_xyz'], bbox['max_xyz'], subject.motion_weights_priors, resolution=resolution,
        level=network.MESH_LEVEL if level is None else level)
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        raise ValueError('run_gltf: the canonical mesh is empty at this level (Network.MESH_LEVEL is not checked on a '
                         'trained checkpoint: pick the level per checkpoint)')
    device = verts.device
    idxs = [subject.framelist.index(f) if isinstance(f, str) else int(f)
            for f in (range(len(subject)) if frames is None else frames)]
    # the subject's priors, uploaded once: Network keeps the weight volume of a resident tensor without comparing it
    priors = torch.as_tensor(subject.motion_weights_priors).to(device=device, dtype=torch.float32)
    first = dict(subject.movement_frame(idxs[0] if idxs else 0, image_size=(1, 1)), motion_weights_priors=priors)
    joints, weights, kept = network.skin_weights(verts, first, k=influences)
    dst_Rs, dst_Ts, Rh, Th, errs = [], [], [], [], []
    for idx in idxs:
        frame = dict(subject.movement_frame(idx, image_size=(1, 1)), motion_weights_priors=priors)
        info = subject.mesh_infos[subject.framelist[idx]]
        rvec = network.refiner_rvec(frame, iter_val)
        dst_Rs.append(gltf.refined_rotations(frame['dst_Rs'], None if rvec is None else rvec.cpu().numpy()))
        dst_Ts.append(frame['dst_Ts'])
        Rh.append(info['Rh'])
        Th.append(info['Th'])
        motion_Rs, motion_Ts, _ = network.frame_motion(frame, iter_val)
        d = skin.skin_lbs(verts, joints, weights, skin.joint_matrices(motion_Rs, motion_Ts)) \
            - network.pose_vertices(verts, frame, iter_val)
        d = torch.sqrt((d * d).sum(1))
        errs.append(torch.stack([d.max(), d.mean()]))
    path = os.path.join(out_dir, 'avatar.glb')
    gltf.write_glb(path, verts, faces, colors, joints, weights, subject.cnl_gtfms,
                   dst_Rs=np.stack(dst_Rs) if idxs else None, dst_Ts=np.stack(dst_Ts) if idxs else None,
                   Rh=np.stack(Rh) if idxs else None, Th=np.stack(Th) if idxs else None, fps=fps, up=up,
                   **(dict(normals=network.vertex_normals(verts, priors, bbox['min_xyz'], bbox['max_xyz'])) if normals else {}))
    per = torch.stack(errs).cpu().numpy().astype(np.float64) if idxs else np.zeros((0, 2))
    return {'path': path, 'V': int(verts.shape[0]), 'F': int(faces.shape[0]), 'frames': idxs,
            'kept': {'min': float(kept.min()), 'mean': float(kept.mean())},
            'skin_error': {'max': float(per[:, 0].max()) if idxs else 0.0, 'mean': float(per[:, 1].mean()) if idxs else 0.0,
                           'per_frame': [{'max': float(a), 'mean': float(b)} for a, b in per]}}


def run_mesh_render(network, subject, kind='movement', resolution=256, level=None, logdir=None, render_folder_name=None,
                    test_num=-1, frame_idx=None, total_frames=None, image_size=None, shade='color', cull='back'):
    """The movement / freeview / tpose sequences as pictures of the posed canonical mesh instead of volume renders: a
    preview (Network.render_mesh: forward skinning, the non-rigid offsets are not inverted; no anti-aliasing).  The mesh
    is extracted once (Network.extract_canonical_mesh as in run_mesh), then every frame of the loop -- camera only, no
    image is loaded -- is posed, rasterised, quantised on the device and written by render.ImageWriter under
    ``<out>/mesh_<kind>/`` (freeview: ``mesh_freeview_<frame_idx>``) with the volume loops' frame names.  Single rank.
    Returns {'frames', 'images', 'image_dir', 'stack'} like the volume loops."""
    import torch
    if kind not in ('movement', 'freeview', 'tpose'):
        raise ValueError("kind must be 'movement', 'freeview' or 'tpose'")
    bbox = subject.canonical_bbox
    verts, faces, colors = network.extract_canonical_mesh(
        bbox['min_xyz'], bbox['max_xyz'], subject.motion_weights_priors, resolution=resolution,
        level=network.MESH_LEVEL if level is None else level)
    # load_image=False: the movement frames carry image_size= and no image
    # src_type=None: freeview_frame is called without src_type (its own default)
    # square_tpose: the T-pose size is int(np.max(image_size)); the volume loops pass image_size through
    # prefix: mesh_<...> folders, which cfg.render_folder_name does not rename
    frames, names, folder = _sequence(subject, kind, load_image=False, test_num=test_num, frame_idx=frame_idx,
                                      total_frames=total_frames, image_size=image_size, src_type=None,
                                      square_tpose=True, prefix='mesh_')
    folder, n = render_folder_name or folder, len(frames)
    device = verts.device
    vout = _VideoOut(os.path.join(_output_dir(logdir), folder), names, 0, 1, device)
    writer = None if vout.only else render.ImageWriter(_output_dir(logdir), folder)
    outbox = render.FrameOutbox(device)
    images, pending = {}, []                # pending: (idx, the outbox's parcel), oldest first

    def hand_over(i, parcel):
        arrs, _, data, _ = parcel.collect()         # the one wait per frame: its copy has landed
        if arrs:
            images[i] = arrs[0]
            writer.append(_panels(*arrs), img_name=names[i])
        if data is not None:
            vout.add(i, data)

    network.eval()
    # the subject's priors, uploaded once: Network keeps the weight volume of a resident tensor without comparing it
    priors = torch.as_tensor(subject.motion_weights_priors).to(device=device, dtype=torch.float32)
    for i in range(n):
        frame = dict(frames[i], motion_weights_priors=priors)
        out = network.render_mesh(verts, faces, colors, frame, iter_val=float(cfg.get('eval_iter', 1e7)),
                                  shade=shade, cull=cull)
        imgs = [render.to_8b_image(out['rgb']), render.to_8b3ch_image(out['alpha']).contiguous()]
        vid = None
        if vout.encoder is not None:
            panels = render.select_panels(imgs[0], imgs[1])
            vid = vout.encoder.encode(panels[0] if len(panels) == 1 else torch.cat(panels, dim=1)) \
                + (imgs[0].shape[0], imgs[0].shape[1] * len(panels))
        pending.append((i, outbox.post([] if vout.only else imgs, video=vid)))
        while len(pending) > 2:                     # two frames in flight: the copy of one overlaps the next raster
            hand_over(*pending.pop(0))
    while pending:
        hand_over(*pending.pop(0))
    stack = writer.finalize() if writer is not None else None
    result = {'frames': list(range(n)), 'images': images, 'image_dir': os.path.join(_output_dir(logdir), folder),
              'stack': stack}
    if vout.encoder is not None:
        result['video'] = vout.finalize()
    return result


def run_surface_points(network, subject, weight_threshold=None, render_folder_name='movement', logdir=None, rank=0,
                       world=1, device=None, test_num=-1):
    """run.py:388-404 (cfg.test.save_3d_together) over the movement frames: one forward per frame with the eleven
    outputs (cfg.amd.diagnostics is switched on for the loop), cloud.surface_records on them, and the records of this
    rank's frames (rank, rank + world, ...) written by ImageWriter.finalize as ``<out>/name-2-3d.bin`` -- with
    world > 1 ``name-2-3d.rank<r>.bin``, to be merged by the caller.  The dict is keyed by the frame name as the
    subject's frame list has it, like the reference's.  ``weight_threshold``: None = cfg.test.weight_threshold, and
    0.3 (the reference's configs/default.yaml:285) where the configuration has no such key.
    Returns {'frames', 'records': {name: CPU tensor [N, 10]}, 'path'}."""
    import torch
    from . import cloud
    device = device or next(network.parameters()).device
    if weight_threshold is None:
        weight_threshold = (cfg.get('test', None) or {}).get('weight_threshold', 0.3)
    frames, _, _ = _sequence(subject, 'movement', device=device, test_num=test_num)
    own = list(range(rank, len(frames), world))
    writer = render.ImageWriter(_output_dir(logdir), render_folder_name, workers=1, keep_frames=False)
    network.eval()
    pre = render.FramePrefetcher(frames, own, device, show_truth=True)
    with _cfg_override(perturb=0., diagnostics=True), contextlib.closing(pre):          # perturb: run.py:214
        for item in pre:
            with torch.no_grad():
                out = network(**item['data'], iter_val=float(cfg.eval_iter))
            rec = cloud.surface_records(out, item['truth'], item['ray_index'], item['W'], weight_threshold)
            writer.append_3d_together(str(subject.framelist[item['idx']]), rec)
    records = dict(writer.name_3d_together)
    writer.finalize()
    path = getattr(writer, 'path_3d_together', None)
    if path is not None and world > 1:
        ranked = path[:-len('.bin')] + '.rank%d.bin' % rank
        os.replace(path, ranked)
        path = ranked
    return {'frames': own, 'records': records, 'path': path}


def run_compare_lbs_delta(network, subject, logdir=None, rank=0, world=1, device=None, test_num=-1):
    """compare_lbs_delta.py of the reference as one loop: every movement frame is rendered twice, with
    cfg.ignore_non_rigid_motions True (LBS only) and then False (the full model), and
    ``<output_dir>/cmp_lbs_delta/movement/{name}_lbs-{s1:.1f}_full-{s2:.1f}.png`` = [lbs render | full render | offset map
    | truth] is written, s1 and s2 the two PSNRs against the truth (compare_lbs_delta.py:21, 36-37, 47-50).  The offset
    map is the geometry panel 'offset' of the full render (sum_s w_s offset_s through the reference's colour map, painted
    where the truth has colour; geometry.frame_maps), so cfg.amd.diagnostics is switched on for the loop.  The PSNRs come
    from MetricsWriter -- ``cmp_lbs_delta/movement_lbs-metrics.perimg.txt`` and ``..._full-...`` are written -- on the
    host, or with cfg.amd.metrics = 'device' from render_frames' device pass.  GPU only.
    Returns {'lbs': [psnr per frame of this rank], 'full': [...], 'names', 'paths', 'image_dir'}."""
    from .config import amd_option, check_amd_options
    check_amd_options()
    device = device or next(network.parameters()).device
    if device.type != 'cuda':
        raise ValueError('run_compare_lbs_delta: the offset map needs a GPU, got device %s' % device)
    on_device = amd_option('metrics', 'host') == 'device'
    frames, names, _ = _sequence(subject, 'movement', device=device, test_num=test_num)
    out_dir = _output_dir(logdir)
    suffix = '' if world == 1 else '.rank%d' % rank
    imgs = {'lbs': {}, 'full': {}}                  # frame -> (render, truth) / -> offset panel
    offset, scores = {}, {}
    with _cfg_override(diagnostics=True, show_truth=True):          # show_truth is put back, unlike run_movement's
        for tag, flag in (('lbs', True), ('full', False)):
            mw = render.MetricsWriter(os.path.join(out_dir, 'cmp_lbs_delta'), 'movement_%s%s' % (tag, suffix),
                                      dataset=subject.dataset_path, metrics=['psnr'])

            def on_image(i, rgb8, alpha8, truth8=None, tag=tag, mw=mw):
                imgs[tag][i] = (rgb8, truth8)
                if truth8 is not None and not on_device:
                    mw.append(name=names[i], pred=rgb8, target=truth8, mask=None)

            extra = {}
            if on_device:
                extra.update(metrics=['psnr'], on_metrics=lambda i, v, mw=mw: mw.append_values(names[i], v))
            if not flag:
                extra.update(maps=['offset'], on_maps=lambda i, panels: offset.__setitem__(i, panels['offset']))
            with _cfg_override(ignore_non_rigid_motions=flag):
                render.render_frames(network, frames, rank=rank, world=world, device=device, on_image=on_image,
                                     show_truth=True, **extra)
            mw.finalize()
            scores[tag] = {k: v['psnr'] for k, v in mw.name2metrics.items()}
    writer = render.ImageWriter(out_dir, os.path.join('cmp_lbs_delta', 'movement'), keep_frames=False)
    own = sorted(imgs['full'])
    paths = []
    for i in own:
        truth = imgs['full'][i][1]
        if truth is None:                           # (a frame without an image has no PSNR and no fourth panel)
            continue
        s1, s2 = scores['lbs'][names[i]], scores['full'][names[i]]
        name = '%s_lbs-%.1f_full-%.1f' % (names[i], s1, s2)
        writer.append(np.concatenate([imgs['lbs'][i][0], imgs['full'][i][0], offset[i], truth], axis=1), img_name=name)
        paths.append(os.path.join(writer.image_dir, name + '.png'))
    writer.finalize()
    return {'lbs': [scores['lbs'][names[i]] for i in own if names[i] in scores['lbs']],
            'full': [scores['full'][names[i]] for i in own if names[i] in scores['full']],
            'names': [names[i] for i in own], 'paths': paths, 'image_dir': writer.image_dir}


def run_distance_matrix(records_or_path, valid_weight_threshold=0.3, dist_thresh=0.002, chunk=(0, 1), method='window',
                        axis=None, logdir=None, out_dir=None, backend='hip', device=None):
    """The main loop of tools/compute_distance*.py on ``name-2-3d.bin`` (a path, or the dict it holds):
    cloud.distance_matrix, saved as ``<out_dir>/distance_mat/distance_mat_{vwt:.2f}-{tau:.2f}[.{chunk_id}-{chunk_n}].npy``
    -- the reference's names, so that its cluster.py reads the file.  ``out_dir``: None = the directory of the records
    file, or the run's output directory for a dict.  Returns {'matrix', 'path', 'names'}."""
    from . import cloud
    records = records_or_path
    if isinstance(records_or_path, (str, os.PathLike)):
        import torch
        records = torch.load(records_or_path, map_location='cpu')
        if out_dir is None:
            out_dir = os.path.dirname(os.path.abspath(records_or_path))
    if out_dir is None:
        out_dir = _output_dir(logdir)
    D = cloud.distance_matrix(records, valid_weight_threshold=valid_weight_threshold, dist_thresh=dist_thresh, chunk=chunk,
                              method=method, axis=axis, backend=backend, device=device)
    path = os.path.join(out_dir, 'distance_mat', cloud.matrix_file_name(valid_weight_threshold, dist_thresh, chunk))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.save(path, D)
    return {'matrix': D, 'path': path, 'names': sorted(records.keys())}


def _load_records(records_or_path, out_dir, logdir):
    """(records, directory to write next to them): a ``name-2-3d.bin`` path or the dict it holds."""
    if isinstance(records_or_path, (str, os.PathLike)):
        import torch
        records = torch.load(records_or_path, map_location='cpu')
        return records, out_dir or os.path.dirname(os.path.abspath(records_or_path))
    return records_or_path, out_dir or _output_dir(logdir)


def run_segments(records_or_path, parts=None, radius=10, image_size=None, logdir=None, out_dir=None, backend='hip',
                 device=None):
    """tools/segment.py on ``name-2-3d.bin`` (a path, or the dict it holds): cloud.segment_records, every part saved as
    ``<out_dir>/name-2-3d.<part>.bin`` -- torch.save of {frame name: tensor [n, 10] or None}, the reference's files, which
    its compute_distance_seg.py and run_distance_matrix read.  ``out_dir``: None = the directory of the records file, or
    the run's output directory for a dict.  Returns {'segments': {part: {...}}, 'paths': {part: path}}."""
    import torch
    from . import cloud
    records, out_dir = _load_records(records_or_path, out_dir, logdir)
    segments = cloud.segment_records(records, parts=parts, radius=radius, image_size=image_size, backend=backend,
                                     device=device)
    os.makedirs(out_dir, exist_ok=True)
    paths = {}
    for part, seg in segments.items():
        paths[part] = os.path.join(out_dir, 'name-2-3d.%s.bin' % part)
        torch.save(seg, paths[part])
    return {'segments': segments, 'paths': paths}


def run_segment_distance_matrices(records_or_path, parts=None, radius=10, image_size=None, valid_weight_threshold=0.3,
                                  dist_thresh=0.002, chunk=(0, 1), axis=None, logdir=None, out_dir=None, backend='hip',
                                  device=None):
    """tools/compute_distance_seg.py for every part, from the UNSEGMENTED ``name-2-3d.bin`` (a path or its dict):
    cloud.segment_distance_matrices, saved as ``<out_dir>/distance_mat_seg/<part>/distance_mat_{vwt:.2f}-{tau:.2f}
    [.{chunk_id}-{chunk_n}].npy``, the reference's tree.  Returns {'matrices': {part: D}, 'paths': {part: path},
    'names'}."""
    from . import cloud
    records, out_dir = _load_records(records_or_path, out_dir, logdir)
    mats = cloud.segment_distance_matrices(records, parts=parts, radius=radius, image_size=image_size,
                                           valid_weight_threshold=valid_weight_threshold, dist_thresh=dist_thresh,
                                           chunk=chunk, axis=axis, backend=backend, device=device)
    paths = {}
    for part, D in mats.items():
        paths[part] = os.path.join(out_dir, 'distance_mat_seg', part,
                                   cloud.matrix_file_name(valid_weight_threshold, dist_thresh, chunk))
        os.makedirs(os.path.dirname(paths[part]), exist_ok=True)
        np.save(paths[part], D)
    return {'matrices': mats, 'paths': paths, 'names': sorted(records.keys())}


def run_cluster(matrix_or_path, names=None, n_clusters=4, out_path=None):
    """tools/cluster.py: cloud.cluster_frames on a distance matrix -- a ``.npy`` path, an array, or what
    run_distance_matrix returned (its 'matrix', 'path' and 'names') -- pickled as the reference does, to the matrix
    path with ``.npy`` replaced by ``.cluster.pkl`` (``out_path`` overrides; an array without either is not written).
    ``names``: the frame names in matrix order, default the sorted record keys of run_distance_matrix's result, else the
    indices.  Returns {'clusters', 'path'}."""
    import pickle
    from . import cloud
    path = None
    if isinstance(matrix_or_path, dict):
        path = matrix_or_path.get('path')
        names = matrix_or_path.get('names') if names is None else names
        D = matrix_or_path['matrix']
    elif isinstance(matrix_or_path, (str, os.PathLike)):
        path = os.fspath(matrix_or_path)
        D = np.load(path)
    else:
        D = matrix_or_path
    clusters = cloud.cluster_frames(D, n_clusters=n_clusters, names=names)
    if out_path is None and path is not None:
        if not path.endswith('.npy'):
            raise ValueError('run_cluster: %r is no .npy matrix file; give out_path' % path)
        out_path = path[:-len('.npy')] + '.cluster.pkl'
    if out_path is not None:
        with open(out_path, 'wb') as f:
            pickle.dump(clusters, f)
    return {'clusters': clusters, 'path': out_path}
