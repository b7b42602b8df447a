"""Configuration for the MI355X-native HumanNeRF hot path.

The reference keeps a process-global yacs singleton ``cfg`` that every module
imports (reference: configs/config.py:58-80, configs/default.yaml).  The hot
path reads only a handful of its keys *at call time* (SURVEY.md section 5):
``N_samples, perturb, chunk, netchunk_per_gpu, ignore_non_rigid_motions,
total_bones, *.kick_in_iter / full_band_iter`` plus the MLP shapes.

Drop-in rule: when this package is loaded inside the reference tree (its
``configs`` package was already imported by train.py / run.py) we use THAT
object, so late mutations such as ``cfg.perturb = 0.`` made by the reference's
drivers (run.py:71,215; trainer.py:181,265) are honoured.  Stand-alone we use
the defaults below, which restate the default.yaml values the path depends on.
"""
import copy
import sys

import yaml


class CfgNode(dict):
    """Minimal attribute-dict config node (own implementation, not yacs)."""

    def __init__(self, init=None):
        super().__init__()
        for k, v in (init or {}).items():
            self[k] = CfgNode(v) if isinstance(v, dict) else v

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = CfgNode(value) if isinstance(value, dict) and not isinstance(value, CfgNode) else value

    def clone(self):
        return copy.deepcopy(self)

    def merge(self, other):
        for k, v in other.items():
            if isinstance(v, dict) and isinstance(self.get(k), dict):
                self[k].merge(v)
            else:
                self[k] = CfgNode(v) if isinstance(v, dict) else v
        return self

    def merge_from_file(self, path):
        with open(path, 'r') as f:
            return self.merge(yaml.safe_load(f) or {})

    def merge_from_list(self, opts):
        """``['a.b', '3', 'c', 'x']`` pairs, values parsed as YAML scalars
        (same convention as the reference CLI, configs/config.py:63)."""
        assert len(opts) % 2 == 0, opts
        for key, val in zip(opts[0::2], opts[1::2]):
            node = self
            parts = key.split('.')
            for p in parts[:-1]:
                node = node[p]
            if parts[-1] not in node:
                raise KeyError(f'unknown config key {key}')
            node[parts[-1]] = yaml.safe_load(val) if isinstance(val, str) else val
        return self


# Values restate configs/default.yaml of the reference (line numbers cited).
_DEFAULTS = {
    'category': 'human_nerf',
    'random_seed': 42,
    'use_amp': False,
    'eval_iter': 10000000,                     # config.py:16
    'ignore_non_rigid_motions': False,         # config.py:20
    'network_module': 'humannerf_amd.network',
    'canonical_mlp': {                         # default.yaml:51-57
        'mlp_depth': 8, 'mlp_width': 256, 'multires': 10, 'i_embed': 0,
        'view_dir': False, 'pose_color': 'wo', 'last_linear_scale': 1,
        'view_embed': 'mlp', 'view_dir_camera_only': False, 'multires_dir': 4,      # default.yaml:58-64
    },
    'mweight_volume': {                        # default.yaml:133-137
        'embedding_size': 256, 'volume_size': 32, 'dst_voxel_size': 0.0625,
    },
    'posevec': {'type': 'axis_angle'},
    'non_rigid_motion_model': 'mlp',
    'non_rigid_motion_mlp': {                  # default.yaml:142-165
        'condition_code_size': 69, 'pose_input': True, 'time_input': False,
        'mlp_width': 128, 'mlp_depth': 6, 'skips': [4], 'multires': 6,
        'i_embed': 0, 'kick_in_iter': 10000, 'full_band_iter': 50000,
        'last_linear_scale': 1,
    },
    'pose_decoder': {                          # default.yaml:237-242
        'embedding_size': 69, 'mlp_width': 256, 'mlp_depth': 4,
    },
    'pose_decoder_off': False,
    'train': {                                 # default.yaml:261-281
        'perturb': 1.0, 'batch_size': 1, 'shuffle': True, 'drop_last': False,
        'maxiter': 400000, 'lr': 0.0005, 'lr_mweight_vol_decoder': 0.00005,
        'lr_pose_decoder': 0.00005, 'lr_non_rigid_mlp': 0.00005,
        'lrate_decay': 500, 'optimizer': 'adam', 'log_interval': 20,
        'save_checkpt_interval': 2000, 'save_model_interval': 50000,
        'ray_shoot_mode': 'patch', 'selected_frame': 'all',
        'lossweights': {'lpips': 1.0, 'mse': 0.2, 'l1': 0.0},
    },
    'sex': 'neutral',
    'total_bones': 24,                         # default.yaml:346
    'bbox_offset': 0.3,                        # default.yaml:347
    'bgcolor': [0., 0., 0.],
    'patch': {'sample_subject_ratio': 0.8, 'N_patches': 6, 'size': 32},
    'N_samples': 128,                          # default.yaml:357
    'perturb': 1.0,                            # default.yaml:359
    'netchunk_per_gpu': 300000,                # default.yaml:361
    'chunk': 32768,                            # default.yaml:362
    'n_gpus': 1,
    # --- keys that exist only in this build -------------------------------
    'amd': {
        # arithmetic of the two per-sample MLPs (inference): 'f16x3' = fp32-equivalent
        # split-f16 (hi+lo) operands, 3 f16 MFMAs, fp32 accumulate -- passes the same
        # parity tests as 'f32' = v_mfma_f32_32x32x2_f32 (bitwise an fp32 fma chain),
        # at 3x the speed.
        'mlp_mode': 'f16x3',
        # arithmetic of the activation-saving training forward ('f32' | 'f16x3')
        'train_mlp_mode': 'f16x3',
        # arithmetic of the weight-gradient kernel for the matrix-shaped layers ('f32' | 'f16x3')
        'train_dw_mode': 'f16x3',
        # arithmetic of the two dX chains ('f32' | 'f16x3')
        'train_chain_mode': 'f16x3',
        # storage of the weight-gradient operands between the kernels of a training step (with split-f16 arithmetic in
        # all three places above): 'f16' = activations and dZ travel as f16 (half the HBM bytes of the step's largest
        # buffers; every product of the weight-gradient sums uses 11-bit operands, fp32 accumulation over >= 10^5
        # samples), 'f32' = fp32 storage, 22-bit split operands in the weight-gradient kernel
        'train_operands': 'f16',
        # every this many backward passes the saved activations and the incoming gradient are checked against the
        # range the split-f16 / f16 arithmetic assumes (autograd.OperandRangeGuard); 0 = never
        'train_check_every': 200,
        # training a multi-head canonical MLP (canonical_mlp.multihead.enable, 2..8 heads of depth 1).  False: such a
        # network is inference only -- Trainer and a training-mode forward raise.  True: a training-mode forward with
        # head_id = h trains head h (the single-head kernels on rows 4h .. 4h+3 of output_linear.0; the other heads' rows
        # get zero gradients), head_id = -1 renders and differentiates every head from one pass through both trunks
        # (include/hnrf_heads_train.h), and Trainer reads batch['head_id'] (dataset.FrameStream: multihead.split)
        'train_heads': False,
        # view-dependent colour (canonical_mlp.view_dir = True, view_embed 'mlp', pose_color 'wo', single head).  False:
        # such a configuration is refused, as every branch outside the default ones.  True: the view branch is built --
        # it has no non-linearity behind the trunk, so it is folded into an ordinary canonical image plus three floats per
        # ray that K4 adds in front of its sigmoid (DESIGN.md section 4 "View-dependent colour"); rendering, baking and
        # training cost what they cost without it.  Network.fixed_view chooses the direction for colour without a ray
        'view_dir': False,
        # inference in 'f16x3' is fp32-accurate for hidden activations below 128 (and clamps them at 65504, the f16
        # range).  The kernels flag any beyond (status word of
        # the packed weight image, read back one frame late without a synchronisation); what Network.forward does when
        # the flag is up: 'raise' ActivationRangeError | 'f32' = warn and render every later frame with the exact fp32
        # MFMA kernels (the flagged frames are wrong: render loops re-render them) | 'ignore'
        'on_f16_range': 'raise',
        # which launches carry the guard (it costs 3 % of a frame): 'audit' = every ray chunk of the first frame after a
        # weight change, then one rotating chunk per frame | 'full' = every chunk of every frame | 'off'
        'f16_range_guard': 'audit',
        # training items of dataset.FrameStream: patch positions drawn with the reference's exact calls on the global
        # numpy generator (True: 4 ms of host time per item) or from a numpy Generator per item (False: 0.1 ms)
        'exact_patch_draws': False,
        # materialise the per-sample diagnostic outputs the reference always
        # returns (backward_motion_weights, xyz_on_rays, ...; ~17 KB/ray).
        'diagnostics': True,
        # cache the motion-weight volume across eval-mode frames while the
        # decoder parameters and the priors tensor are unchanged.
        'cache_weight_volume': True,
        # inference only: where a sample's raw (r, g, b, sigma) comes from.  'mlp' = the canonical MLP (the reference).
        # 'baked' = an opt-in approximation: the MLP tabulated once per checkpoint on a bake_resolution^3 f16 lattice over
        # the canonical bbox and interpolated trilinearly per sample (Network.bake_canonical / set_baked_grid,
        # DESIGN.md section 4 "Baked canonical grid"); everything else of the frame stays exact.  Training ignores it;
        # term_eps > 0 in the lean form is refused with it
        'canonical': 'mlp',
        'bake_resolution': 256,
        # inference only, and only with canonical = 'baked': where a sample's non-rigid offset comes from.  'mlp' = the
        # non-rigid motion MLP (the reference).  'baked' = an opt-in approximation: within a frame the offset is a
        # function of x_skel alone, so it is tabulated once per FRAME on a nonrigid_bake_resolution^3 f16 lattice over the
        # canonical bbox (Network.bake_nonrigid) and interpolated trilinearly per sample in one kernel with the canonical
        # grid's look-up (DESIGN.md section 4 "Baked non-rigid offset field").  Training and ignore_non_rigid_motions
        # ignore it; with canonical = 'mlp' it is refused
        'nonrigid': 'mlp',
        'nonrigid_bake_resolution': 128,
        # lean rendering only: skip the MLPs for samples whose foreground likelihood (sum of
        # skinning weights) is below this; bounds |d rgb|, |d alpha| by ~2 * N_samples * cull_eps.
        # 0 = evaluate every sample exactly like the reference.  1e-9 already drops ~55 % of the
        # samples of a typical frame at an error 100x below the reference's own fp32 noise.
        'cull_eps': 0.0,
        # lean rendering only: stop evaluating a ray once its transmittance is below this (front-to-back slabs of 32
        # samples); bounds |d rgb|, |d alpha| by term_eps.  0 = off (the reference evaluates every sample).
        'term_eps': 0.0,
        # rendering: run the LBS warp (K1) of ray chunk i+1 on a side stream while the MLP kernels of chunk i occupy
        # the main one (ordering by events inside hnrf_render_frame_fwd, no host synchronisation).  Measured on the
        # 512x512x128 frame: 91.5 ms with and without it -- the MLP kernels are power-limited, so whatever K1 draws
        # beside them they lose; off by default
        'overlap_warp': False,
        # dense inference in 'f16x3' with cull_eps == 0: samples whose x_skel is so small that the split-f16 operands of
        # the non-rigid MLP are those of x_skel = 0, and whose x_skel + offset rounds to the offset, share ONE evaluation
        # of both MLPs per frame (the predicate: include/hnrf.h, hnrf_share_compact; DESIGN.md "Shared underflowing
        # inputs").  Bit-identical outputs; False = the launches without it
        'share_underflow': True,
        # multi-GPU training: 'volume' = average the 3.3 MB weight-volume gradient in front of the decoder backward (the
        # decoder's 254 MB of gradients never travel; needs the same priors on every rank, verified at run time),
        # 'full' = plain all-reduce of every gradient
        'ddp_reduce': 'volume',
        # run the collectives of the training step even when world_size == 1 (identities over a one-rank group):
        # exercises the RCCL code path on a single-GPU box (tests/test_gpu_dist.py)
        'ddp_single_rank_collectives': False,
        # run.run_movement: where the per-image PSNR / SSIM / LPIPS are computed.  'host' = MetricsWriter.append on the
        # images that arrived on the host (the reference's route: scipy / torch on the thread that drives the GPU),
        # 'device' = in the frame's own launches on the 8-bit device images (render_frames(metrics=...): exact integer
        # moments, hnrf_image_metrics), the values travelling behind the images; needs a GPU
        'metrics': 'host',
        # run.run_movement / run_freeview / run_tpose / run_mesh_render: a Motion-JPEG video of the panels next to the PNGs.
        # 'none' = nothing changes; 'mjpeg' = every frame's panels are JPEG-encoded on the device in the frame's launches
        # (humannerf_amd/video.py, csrc/hnrf_video.hip) and written as <image_dir>.avi (.rank<r>.avi with world > 1:
        # video.merge_parts joins them); 'mjpeg_only' = the video alone: no 8-bit image is copied to the host, no PNG is
        # written (with metrics it needs metrics = 'device')
        'video': 'none',
        'video_quality': 90,              # 1 .. 100, the scale of PIL.Image.save(quality=)
        'video_fps': 10,                  # integer >= 1; 10 as the reference's ImageWriter.finalize
        # the render loops of run.py: geometry panels next to the colour image, a list out of 'depth', 'normal', 'shaded',
        # 'offset' (humannerf_amd/geometry.py, csrc/hnrf_geometry.hip: screen-space differences of the rendered surface
        # distance, computed in the frame's launches; GPU only).  [] = nothing changes.  'offset' -- the colour map of the
        # weighted non-rigid offset, compare_lbs_delta.py of the reference -- needs diagnostics = True
        'maps': [],
        # the surface distance the maps are made of: 'expected' = depth / alpha, 'median' = the depth of the sample where
        # the cumulative weight reaches half of its total (needs diagnostics = True)
        'maps_surface': 'expected',
        # where the 'normal' and 'shaded' panels take their normals from: 'screen' = differences of the rendered surface
        # distance (nothing changes); 'gradient' = the gradient of the density at the ray's samples (Network.ray_normals,
        # include/hnrf_normals.h: the training kernels run over the kept samples; one device count is read back per
        # frame).  'gradient' needs diagnostics = True
        'maps_normals': 'screen',
        # 'gradient': a sample takes part in its ray's normal iff its compositing weight is >= this; finite and > 0
        'normal_weight_min': 1e-4,
        # gc.freeze() at the start of the training / render loops (config.quiet_gc)
        'freeze_gc': True,
    },
}


# The top-level ``multihead`` node beside its head_num (default.yaml:372-382).  The node as a whole has no default here
# (a config without it selects no multi-head network: network.canonical_head_num); these are what multihead_option
# answers for a key the node does not carry.
MULTIHEAD_DEFAULTS = {
    'split': 'view',                                   # 'view' | 'random' | 'argmin' | path of a JSON {frame_name: head}
    'argmin_cfg': {'selector_criteria': {'lpips': 1.0, 'mse': 0.2, 'ssim': 0.0},
                   'unselected_lossweights': {'lpips': 0.0, 'mse': 0.0}},
}


def multihead_option(path, config=None):
    """``multihead.<path>`` ('split', 'argmin_cfg.selector_criteria', ...) of ``config`` (default: cfg), with
    MULTIHEAD_DEFAULTS where the node or the key is missing."""
    def walk(node):
        for part in path.split('.'):
            if not hasattr(node, 'get') or node.get(part, None) is None:
                return None
            node = node[part]
        return node
    config = cfg if config is None else config
    got = walk(config.get('multihead', None) if hasattr(config, 'get') else None)
    return walk(MULTIHEAD_DEFAULTS) if got is None else got


_GC_FROZEN = False


def quiet_gc():
    """Take the objects that exist now (modules, the network, the autograd / ctypes machinery: ~10^6 of them) out of the
    cyclic garbage collector's generations.  A full collection otherwise walks all of them every few thousand
    allocations: measured 90-100 ms once per ~138 training steps (0.65 ms per step, 5 %) and the same stall at random
    places in a render loop.  Called once per process by the loops of train.py / render.py and by bench.py; the collector
    stays enabled for what is allocated afterwards.  cfg.amd.freeze_gc = False turns it off."""
    global _GC_FROZEN
    if _GC_FROZEN or not amd_option('freeze_gc', True):
        return
    import gc
    gc.collect()
    gc.freeze()
    _GC_FROZEN = True


def get_cfg_defaults():
    return CfgNode(_DEFAULTS)


def _resolve_cfg():
    ref = sys.modules.get('configs')
    if ref is not None and hasattr(ref, 'cfg'):
        return ref.cfg           # reference singleton: drop-in mode
    return get_cfg_defaults()


cfg = _resolve_cfg()


def check_amd_options(node=None):
    """Validate the options of the two baked approximations that go together (``node``: an ``amd`` mapping, default
    cfg.amd) and return (canonical, nonrigid, nonrigid_bake_resolution).  ValueError: a value that is not 'mlp' or
    'baked', a resolution that is no integer in [8, 512], nonrigid = 'baked' without canonical = 'baked', or a
    share_underflow that is no bool, or a metrics route that is not 'host' or 'device', or a video option out of range
    (video 'none' / 'mjpeg' / 'mjpeg_only', video_quality an integer in [1, 100], video_fps an integer >= 1), or
    video = 'mjpeg_only' with metrics = 'host' (the host route needs the images that mode does not copy), or maps that
    is no list of distinct names out of 'depth' / 'normal' / 'shaded' / 'offset', a maps_surface that is not 'expected' or
    'median', or 'offset' / 'median' asked for with diagnostics off, or a maps_normals that is not 'screen' or
    'gradient', a normal_weight_min that is not finite and > 0, or 'gradient' with diagnostics off."""
    get = amd_option if node is None else (lambda k: node.get(k, _DEFAULTS['amd'][k]))
    if not isinstance(get('share_underflow'), bool):
        raise ValueError('cfg.amd.share_underflow must be True or False, got %r' % (get('share_underflow'),))
    if get('metrics') not in ('host', 'device'):
        raise ValueError("cfg.amd.metrics must be 'host' or 'device', got %r" % (get('metrics'),))
    video, vq, fps = get('video'), get('video_quality'), get('video_fps')
    if video not in ('none', 'mjpeg', 'mjpeg_only'):
        raise ValueError("cfg.amd.video must be 'none', 'mjpeg' or 'mjpeg_only', got %r" % (video,))
    if isinstance(vq, bool) or not isinstance(vq, int) or not 1 <= vq <= 100:
        raise ValueError('cfg.amd.video_quality must be an integer in [1, 100], got %r' % (vq,))
    if isinstance(fps, bool) or not isinstance(fps, int) or fps < 1:
        raise ValueError('cfg.amd.video_fps must be an integer >= 1, got %r' % (fps,))
    if video == 'mjpeg_only' and get('metrics') == 'host':
        raise ValueError("cfg.amd.video = 'mjpeg_only' copies no image to the host, so cfg.amd.metrics = 'host' cannot "
                         "compute anything: set cfg.amd.metrics = 'device' or cfg.amd.video = 'mjpeg'")
    maps, surface = get('maps'), get('maps_surface')
    if not isinstance(maps, (list, tuple)) or any(m not in ('depth', 'normal', 'shaded', 'offset') for m in maps) \
            or len(set(maps)) != len(maps):
        raise ValueError("cfg.amd.maps must be a list of distinct names out of 'depth', 'normal', 'shaded', 'offset', got %r"
                         % (maps,))
    if surface not in ('expected', 'median'):
        raise ValueError("cfg.amd.maps_surface must be 'expected' or 'median', got %r" % (surface,))
    if not get('diagnostics') and maps and ('offset' in maps or surface == 'median'):
        raise ValueError("cfg.amd.maps with 'offset', and cfg.amd.maps_surface = 'median', need cfg.amd.diagnostics = True "
                         "(got cfg.amd.maps = %r, cfg.amd.maps_surface = %r): the lean form returns neither the per-sample "
                         "weights nor the offsets" % (list(maps), surface))
    normals, wmin = get('maps_normals'), get('normal_weight_min')
    if normals not in ('screen', 'gradient'):
        raise ValueError("cfg.amd.maps_normals must be 'screen' or 'gradient', got %r" % (normals,))
    if isinstance(wmin, bool) or not isinstance(wmin, (int, float)) or not (wmin > 0 and wmin < float('inf')):
        raise ValueError('cfg.amd.normal_weight_min must be finite and > 0, got %r' % (wmin,))
    if normals == 'gradient' and not get('diagnostics'):
        raise ValueError("cfg.amd.maps_normals = 'gradient' needs cfg.amd.diagnostics = True (got cfg.amd.maps = %r): the "
                         "lean form returns neither the per-sample weights nor the bone weights" % (list(maps),))
    canonical, nonrigid, M = get('canonical'), get('nonrigid'), get('nonrigid_bake_resolution')
    if canonical not in ('mlp', 'baked'):
        raise ValueError("cfg.amd.canonical must be 'mlp' or 'baked', got %r" % (canonical,))
    if nonrigid not in ('mlp', 'baked'):
        raise ValueError("cfg.amd.nonrigid must be 'mlp' or 'baked', got %r" % (nonrigid,))
    if isinstance(M, bool) or not isinstance(M, int) or not 8 <= M <= 512:
        raise ValueError('cfg.amd.nonrigid_bake_resolution must be an integer in [8, 512], got %r' % (M,))
    if nonrigid == 'baked' and canonical != 'baked':
        raise ValueError("cfg.amd.nonrigid = 'baked' needs cfg.amd.canonical = 'baked' (got cfg.amd.canonical = %r): "
                         "the offset grid is sampled in one kernel with the canonical grid" % (canonical,))
    return canonical, nonrigid, M


def amd_option(name, default=None):
    """Read a build-specific option; the reference cfg has no ``amd`` node."""
    node = cfg.get('amd', None) if hasattr(cfg, 'get') else None
    if node is None:
        return _DEFAULTS['amd'].get(name, default)
    return node.get(name, _DEFAULTS['amd'].get(name, default))
