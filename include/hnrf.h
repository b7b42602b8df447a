/*
 * hnrf.h -- C ABI of the MI355X-native HumanNeRF ray-marching path
 * (libhnrf.so, hand-written HIP for gfx950).
 *
 * The reference (ChenYutongTHU/humannerf) is pure Python/PyTorch and has no FFI;
 * its "operator interface" for this path is the set of methods of
 * core/nets/human_nerf/network.py::Network.  Each entry point below replaces
 * the torch-op sequence of one of those methods and cites it.  A maintainer of
 * the reference binds these with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions:
 *  - every pointer is a DEVICE pointer to contiguous row-major fp32 unless
 *    stated otherwise; the caller owns every buffer, the library allocates
 *    nothing and keeps no state between calls;
 *  - `stream` is a hipStream_t passed as void*; calls are stream-ordered and
 *    never synchronise the device or touch the host copy of any buffer;
 *  - return value 0 = success, negative = error (see HNRF_E_*); the message is
 *    available from hnrf_last_error() (thread-local); nothing throws or exits;
 *  - nullable outputs may be passed as NULL to skip their HBM writes.
 */
#ifndef HNRF_H
#define HNRF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HNRF_OK            0
#define HNRF_E_ARG        -1   /* null pointer / bad dimension            */
#define HNRF_E_UNSUPPORTED -2  /* layer shape / mode not built            */
#define HNRF_E_LAUNCH     -3   /* hipLaunch / hipGetLastError failed      */
#define HNRF_E_WORKSPACE  -4   /* workspace too small                     */

/* arithmetic of the per-sample MLP GEMMs */
#define HNRF_MLP_F32    0      /* v_mfma_f32_32x32x2_f32: exact fp32 fma chain   */
#define HNRF_MLP_F16X3  1      /* split-fp16 (hi+lo) inputs, 3 MFMAs, fp32 accum */
#define HNRF_MLP_F16X3_H 2     /* training entry points only (hnrf_*_fwd_train, hnrf_*_bwd): HNRF_MLP_F16X3 arithmetic with
                                * the saved weight-gradient operands in f16 -- acts / dZ are f16 matrices of the same
                                * layer count in the BLOCKED layout of hnrf_mlp_dw_h (every layer padded to a multiple of 128
                                * samples: [L][ceil(P / 128) * 128][width]), pe_out is row-major f16 [P][64] (zero-padded), dZ
                                * carries the chain's power-of-two scale and dz_amax receives that scale per layer ([L]
                                * floats) for hnrf_mlp_dw_h.  Packed images are the HNRF_MLP_F16X3 ones. */

int         hnrf_abi_version(void);
const char* hnrf_last_error(void);

/* ---- f16-range guard of the HNRF_MLP_F16X3 inference kernels ------------------
 * The split v = hi + lo only holds below 65504: the kernels clamp post-ReLU activations there, so a checkpoint whose
 * hidden activations leave the f16 range would render a wrong image without any error (the reference's fp32 nn.Linear
 * chains, mlp_rgb_sigma.py:163-198 / mlp_offset.py:74-84, have no such limit).  Every packed image therefore carries a
 * STATUS WORD (uint32 at byte offset hnrf_*_status_offset(mode) of the caller's `packed` buffer; zeroed by every
 * hnrf_*_pack): hnrf_canonical_fwd / hnrf_nonrigid_fwd, their sparse forms and the hnrf_render_* entries OR
 * HNRF_STATUS_F16_RANGE into it when any activation reached 128.  This is the one place where a forward call
 * writes into `packed`.  The caller reads the word when it likes (no call synchronises) and re-renders with
 * HNRF_MLP_F32, which has no such limit (offset 0 = the mode has no status word).  Training has its own guard on
 * the saved activations (humannerf_amd/autograd.py OperandRangeGuard).
 * Why 128 and not the f16 range: the forward images store a weight's low part un-lifted, w = hi + f16(w - hi), so a
 * weight below 0.25 keeps an absolute error of up to 2^-25 and an activation a turns it into up to |a| 2^-25 per
 * product.  An activation carried into the output by small weights (tests/test_gpu_f16_range.py) stays fp32-accurate
 * up to 100 and is off by 2.3e-5 of the output at 1e3, 6.8e-4 at 5e4.  The contract: no report -> fp32 accuracy. */
#define HNRF_STATUS_F16_RANGE 1u
size_t hnrf_canonical_status_offset(int mode);
size_t hnrf_nonrigid_status_offset(int mode);
/* The guard costs 5 VALU instructions per 8 activations (+2.5 % canonical-kernel time, -3.0 % rays/s on the
 * 512x512x128 frame, measured A/B).  Flags OR-ed into the `mode` argument of the forward entry points select unguarded
 * kernel instances; the low byte stays the arithmetic:
 *   (none)                       every launch is guarded (the default of every entry point);
 *   HNRF_MLP_NO_RANGE_GUARD      no launch is guarded -- the status words stay as they are;
 *   HNRF_MLP_GUARD_ONE_CHUNK     hnrf_render_frame_fwd only: of the frame's ray chunks only number
 *                                ((unsigned)mode >> 16) % n_chunks is guarded -- the caller rotates that index from
 *                                frame to frame (an audit: humannerf_amd.network guards every chunk of the first frame
 *                                after a weight change and one rotating chunk afterwards, cfg.amd.f16_range_guard). */
#define HNRF_MLP_ARITH_MASK       0xff
#define HNRF_MLP_NO_RANGE_GUARD   0x100
#define HNRF_MLP_GUARD_ONE_CHUNK  0x200

/* ---- K1: z-sampling + inverse-LBS warp ------------------------------------
 * Replaces Network._get_samples_along_ray / _stratified_sampling
 * (network.py:455-471), pts = o + d*z (network.py:499) and
 * Network._sample_motion_fields (network.py:392-444).
 *  rays_o, rays_d [R,3]; near, far [R]; t_rand [R,S] or NULL (perturb == 0);
 *  motion_Rs [B,3,3], motion_Ts [B,3]; vol [>=B, G,G,G] (background channel, if
 *  present, is not read); bbox_min, bbox_scale [3]   -- all device pointers.
 * Outputs: z_vals [R,S], x_skel [R,S,3], fg_mask [R,S] (= sum of weights,
 *  unclamped), bmw [R,S,B] or NULL (unnormalised per-bone weights; with
 *  B == 24 16-byte aligned -- it is then written in 16-byte pieces --,
 *  HNRF_E_ARG otherwise).
 * Every operation of the reference's tensor expressions is rounded on its own
 * (no compiler-chosen fma), so all forms of the kernel agree bit for bit.
 * z_vals: torch.linspace's element in its two forms, step * s below the midpoint
 * S / 2 and 1 - step * (S - 1 - s) from it on, step = 1 / (S - 1) in fp32; equal
 * bit for bit to that statement (tests/test_render_kernel_refs.py::
 * z_statement_fp32), within an ulp of torch.linspace's own kernels.
 * Limits, checked before any launch (HNRF_E_ARG): S >= 2, B >= 1, 2 <= G <= 1024,
 * bmw 16-byte aligned when B == 24 (any other B: 4-byte stores, no requirement).
 * R == 0 returns HNRF_OK without a launch and leaves every output untouched. */
int hnrf_sample_warp_fwd(const float* rays_o, const float* rays_d,
                         const float* near, const float* far, const float* t_rand,
                         const float* motion_Rs, const float* motion_Ts,
                         const float* vol, const float* bbox_min, const float* bbox_scale,
                         int64_t R, int S, int B, int G,
                         float* z_vals, float* x_skel, float* fg_mask, float* bmw,
                         void* stream);

/* ---- sample culling (no counterpart in the reference, which evaluates every sample) --------
 * idx[0 .. *count) = indices p with fg_mask[p] >= eps, count written on the device (no host
 * sync).  alpha = (1 - exp(-sigma delta)) * fg_mask (network.py:369) < eps for a dropped sample,
 * so a ray's rgb / alpha / depth move by at most ~2 S eps; eps == 0 keeps every sample and the
 * path is exactly the reference's.  idx must hold P ints; idx[*count .. P) is NOT written (it keeps what it
 * held); a NaN fg_mask is never kept, also at eps == 0; P < 2^31 - 1; P == 0 sets *count = 0 without a launch. */
int hnrf_compact_samples(const float* fg_mask, float eps, int64_t P, int* idx, int* count, void* stream);

/* ---- K2: non-rigid motion MLP ---------------------------------------------
 * Replaces hannw_fourier embed (embedders/hannw_fourier.py:21-49) +
 * NonRigidMotionMLP.forward (non_rigid_motion_mlps/mlp_offset.py:74-114) as
 * called from Network._apply_mlp_kernals (network.py:264-275).
 * Default architecture only: 6 x 128, skip [h | PE36] at layer 4, out 3,
 * condition code 69 (one vector per frame, folded into the first bias).
 *
 * hnrf_nonrigid_pack: weights[7], biases[7] are the nn.Linear tensors
 *  block_mlps.{0,2,...,12} in (out,in) layout; cond [69] is the (possibly
 *  zeroed, network.py:735-737) condition code.  Writes the MFMA-ordered weight
 *  image into `packed` (hnrf_nonrigid_packed_bytes(mode) bytes).  Re-run after
 *  every parameter update or new frame (cond changes per frame). */
size_t hnrf_nonrigid_packed_bytes(int mode);
int hnrf_nonrigid_pack(const float* const* weights, const float* const* biases,
                       const float* cond, int mode, void* packed, void* stream);
/*  x_skel [P,3]; hann_w [6] device pointer (window weights, hannw_fourier.py:
 *  26-40).  Outputs xyz = x_skel + offset [P,3]; offsets [P,3] or NULL. */
int hnrf_nonrigid_fwd(const float* x_skel, const float* hann_w, const void* packed,
                      int mode, int64_t P, float* xyz, float* offsets, void* stream);
/*  Sparse form, as hnrf_canonical_fwd_sparse below: xyz (and offsets) are written at the listed samples only. */
int hnrf_nonrigid_fwd_sparse(const float* x_skel, const float* hann_w, const void* packed,
                             int mode, int64_t P, const int* idx, const int* count,
                             float* xyz, float* offsets, void* stream);

/* ---- K3: canonical MLP ----------------------------------------------------
 * Replaces fourier embed (embedders/fourier.py:9-38) + CanonicalMLP.forward
 * default branch (canonical_mlps/mlp_rgb_sigma.py:132-198) as called from
 * Network._apply_mlp_kernals (network.py:305-315).
 * Default architecture only: PE63 -> 8 x 256, skip [PE63 | h] at layer 5, out 4.
 *  weights[9], biases[9]: pts_linears.{0,...,14} then output_linear.0. */
size_t hnrf_canonical_packed_bytes(int mode);
int hnrf_canonical_pack(const float* const* weights, const float* const* biases,
                        int mode, void* packed, void* stream);
/*  xyz [P,3] -> raw [P,4] = (r,g,b,sigma) pre-activation. */
int hnrf_canonical_fwd(const float* xyz, const void* packed, int mode, int64_t P,
                       float* raw, void* stream);
/*  Sparse form: only the samples idx[0 .. *count) are evaluated (xyz read at and raw written to
 *  those indices; everything else untouched, and the listed rows equal the dense launch bit for bit).  idx, count:
 *  device pointers from hnrf_compact_samples; P = capacity of idx (grid size), *count <= P is read on the device;
 *  idx[*count .. P) is not read; *count == 0 writes nothing. */
int hnrf_canonical_fwd_sparse(const float* xyz, const void* packed, int mode, int64_t P,
                              const int* idx, const int* count, float* raw, void* stream);

/* ---- K4: alpha compositing --------------------------------------------------
 * Replaces Network._raw2outputs (network.py:355-388).
 *  raw [R,S,4]; fg_mask [R,S]; z_vals [R,S]; rays_d [R,3]; xyz [R,S,3] (may be
 *  NULL when cnl_xyz is NULL); bgcolor [3] in 0..255 (device pointer).
 *  cull_eps: samples with fg_mask < cull_eps get weight 0 and their raw is not interpreted
 *  (0 = reference behaviour).
 * Outputs: rgb [R,3], alpha [R], depth [R]; nullable: weights [R,S],
 *  rgb_on_rays [R,S,3] (0 at culled samples), cnl_xyz [R,3], cnl_rgb [R,3], cnl_weight [R]: gathered at the
 *  largest weight of the ray, of equal weights at the first (a ray without any weight: sample 0).
 * Limits: 2 <= S <= 512 (HNRF_E_UNSUPPORTED above 512), raw 16-byte aligned (HNRF_E_ARG). */
int hnrf_composite_fwd(const float* raw, const float* fg_mask, const float* z_vals,
                       const float* rays_d, const float* xyz, const float* bgcolor,
                       int64_t R, int S, float cull_eps,
                       float* rgb, float* alpha, float* depth,
                       float* weights, float* rgb_on_rays,
                       float* cnl_xyz, float* cnl_rgb, float* cnl_weight,
                       void* stream);

/* ---- whole path for one ray chunk -------------------------------------------
 * Replaces Network._render_rays (network.py:474-602): K1 -> K2 -> K3 -> K4 on
 * `stream`, intermediates in caller-provided workspace
 * (hnrf_render_workspace_bytes(R,S) bytes, 256-byte aligned).
 * nr_packed == NULL means cfg.ignore_non_rigid_motions (network.py:264,276-277).
 * cull_eps > 0: the MLPs run only on the samples with fg_mask >= cull_eps (see
 * hnrf_compact_samples); 0 = every sample, as the reference.
 * Only rgb/alpha/depth are written (the trainer and the image writers read
 * nothing else: trainer.py:121, run.py:130).
 * ev_mlp_start / ev_mlp_stop: optional hipEvent_t (as void*, may be NULL) recorded
 * on `stream` right before / after the canonical-MLP launch, so a caller can time
 * the dominant kernel without a profiler (bench.py roofline). */
size_t hnrf_render_workspace_bytes(int64_t R, int S);
int hnrf_render_rays_fwd(const float* rays_o, const float* rays_d,
                         const float* near, const float* far, const float* t_rand,
                         const float* motion_Rs, const float* motion_Ts,
                         const float* vol, const float* bbox_min, const float* bbox_scale,
                         const float* hann_w, const void* nr_packed, const void* cnl_packed,
                         const float* bgcolor, int mode, float cull_eps,
                         int64_t R, int S, int B, int G,
                         void* workspace, size_t workspace_bytes,
                         float* rgb, float* alpha, float* depth,
                         void* ev_mlp_start, void* ev_mlp_stop, void* stream);

/* Opt-in variant with early ray termination (NOT the reference arithmetic): the samples are walked front to back
 * in slabs of 32; a ray whose transmittance has fallen below term_eps (0 < term_eps < 1) is not evaluated further,
 * which moves rgb / alpha by at most term_eps; cull_eps as above (may be 0).  evaluated (nullable): device int that
 * receives the number of samples that went through the MLPs.  workspace: hnrf_render_term_workspace_bytes.
 * Exactly: a ray is alive for a slab iff its transmittance BEFORE that slab is >= term_eps (so the slab in which it
 * falls under the threshold is still composited whole); a sample is evaluated iff its ray is alive and fg_mask >=
 * cull_eps (at cull_eps == 0 that includes fg_mask == 0); every other sample enters with alpha = 0. */
size_t hnrf_render_term_workspace_bytes(int64_t R, int S);
int hnrf_render_rays_term_fwd(const float* rays_o, const float* rays_d,
                              const float* near, const float* far, const float* t_rand,
                              const float* motion_Rs, const float* motion_Ts,
                              const float* vol, const float* bbox_min, const float* bbox_scale,
                              const float* hann_w, const void* nr_packed, const void* cnl_packed,
                              const float* bgcolor, int mode, float cull_eps, float term_eps,
                              int64_t R, int S, int B, int G,
                              void* workspace, size_t workspace_bytes,
                              float* rgb, float* alpha, float* depth, int* evaluated, void* stream);

/* Whole frame: Network._batchify_rays (network.py:330-352) over _render_rays.  N rays in chunks of `chunk` (cfg.chunk)
 * through K1..K4, rgb [N,3] / alpha [N] / depth [N] written for the whole frame.  The eight diagnostic outputs of the
 * reference's forward are optional, all or none (whole-frame buffers: weights_on_rays [N,S], rgb_on_rays [N,S,3],
 * cnl_xyz [N,3], cnl_rgb [N,3], cnl_weight [N], xyz_on_rays [N,S,3], bmw [N,S,B], offsets [N,S,3]); sample culling
 * (cull_eps > 0) only without them.  workspace: hnrf_render_frame_workspace_bytes(chunk, S), 256-byte aligned (two chunk
 * workspaces that alternate).
 * side_stream (nullable): a second stream of the same device on which the LBS warp (K1) of chunk i+1 runs while the
 * MLP kernels of chunk i occupy `stream` -- K1 has no LDS and few registers, so it shares the CUs with them.  Needs
 * events = 5 hipEvent_t owned by the caller (no timing needed); all ordering between the two streams is expressed
 * through them, nothing is synchronised with the host.  On return every result is ordered on `stream`.
 * mlp_events (nullable): 2 x ceil(N / chunk) hipEvent_t recorded around every canonical-MLP launch (for timing). */
size_t hnrf_render_frame_workspace_bytes(int64_t chunk, int S);
int hnrf_render_frame_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                          const float* t_rand, const float* motion_Rs, const float* motion_Ts, const float* vol,
                          const float* bbox_min, const float* bbox_scale, const float* hann_w, const void* nr_packed,
                          const void* cnl_packed, const float* bgcolor, int mode, float cull_eps, int64_t N, int S,
                          int B, int G, int64_t chunk, void* workspace, size_t workspace_bytes, float* rgb, float* alpha,
                          float* depth, float* weights_on_rays, float* rgb_on_rays, float* cnl_xyz, float* cnl_rgb,
                          float* cnl_weight, float* xyz_on_rays, float* bmw, float* offsets, void* side_stream,
                          void* const* events, void* const* mlp_events, void* stream);

/* ---- samples whose MLP inputs underflow to those of x_skel = 0 (HNRF_MLP_F16X3 only) --------
 * Far from every bone K1 leaves x_skel ~ 1e-16: tiny, rarely zero.  K2's split-f16 B operand cannot tell such a value
 * from zero -- its positional encoding is hann_k sin(2^k x), at most 32 |x| while every hann_k <= 1, whose f16 high and
 * low parts are both +-0 below 2^-25, and its cosines are exactly 1 -- so the offset is the per-frame constant
 * c_off = K2(+0, +0, +0); where x_skel + c_off also rounds to c_xyz = +0 + c_off, K3 sees the representative's bits too
 * and raw is the constant c_raw.  THE PREDICATE: a sample is SHARED when for a = 0..2
 *   (a) |x_skel[a]| <= HNRF_SHARE_T, and
 *   (b) the bits of x_skel[a] + c_off[a] (one rounded fp32 add, K2's own) equal the bits of c_xyz[a];
 * a NaN or infinite coordinate fails (a).  HNRF_SHARE_T = 2^-31 leaves a factor 2 under the f16 tie at 2^-25 for the
 * top octave and holds only while every Hann weight is <= 1 -- the CALLER checks that before it uses these entries.
 *
 * hnrf_share_compact: idx[0 .. *count) = the samples p < P that are NOT shared (order as hnrf_compact_samples; count is
 *  zeroed and written on the device, idx[*count .. P) keeps what it held), and for every shared p: raw[p] = c_raw [4],
 *  offsets[p] = c_off [3], xyz[p] = c_xyz [3] (offsets and xyz both NULL = not written); the rows of live samples are
 *  not touched.  c_off / c_xyz / c_raw: device pointers, what K2 and K3 wrote for x_skel = (+0, +0, +0).
 *  raw 16-byte aligned, P < 2^31 - 1; P == 0 sets *count = 0 without a launch. */
#define HNRF_SHARE_T 4.656612873077392578125e-10f
int hnrf_share_compact(const float* x_skel, const float* c_off, const float* c_xyz, const float* c_raw, int64_t P,
                       int* idx, int* count, float* offsets, float* xyz, float* raw, void* stream);
/* The same classification inside K1 (24 bones only: HNRF_E_UNSUPPORTED otherwise), on the x_skel values the block
 * still holds in registers: no second pass over x_skel, and the one atomic per block of 256 samples waits under the
 * arithmetic of the CU's other resident blocks.  Arguments through bmw as hnrf_sample_warp_fwd, and z_vals / x_skel /
 * fg_mask / bmw are written exactly as there; c_off .. raw as hnrf_share_compact, with P = R S < 2^31 - 1. */
int hnrf_sample_warp_share_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                               const float* t_rand, const float* motion_Rs, const float* motion_Ts, const float* vol,
                               const float* bbox_min, const float* bbox_scale, int64_t R, int S, int B, int G,
                               float* z_vals, float* x_skel, float* fg_mask, float* bmw, const float* c_off,
                               const float* c_xyz, const float* c_raw, int* idx, int* count, float* offsets, float* xyz,
                               float* raw, void* stream);
/* hnrf_render_frame_fwd with every chunk as K1 with the classification fused in (hnrf_sample_warp_share_fwd; any bone
 * count but 24: K1 -> hnrf_share_compact) -> K2 and K3 on the live list -> K4, the
 * representative evaluated once per frame in front of chunk 0 by the same kernel instances (guarded unless
 * HNRF_MLP_NO_RANGE_GUARD; no mlp_events around it, the pairs stay one per chunk, around K3 on the live list).  Every
 * output equals hnrf_render_frame_fwd's bit for bit.  live_counts [ceil(N / chunk)] (device, required): receives the
 * number of samples of each chunk that went through the MLPs.  HNRF_E_UNSUPPORTED unless mode is HNRF_MLP_F16X3,
 * nr_packed is given and cull_eps == 0.  workspace: hnrf_render_frame_shared_workspace_bytes(chunk, S). */
size_t hnrf_render_frame_shared_workspace_bytes(int64_t chunk, int S);
int hnrf_render_frame_shared_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                 const float* t_rand, const float* motion_Rs, const float* motion_Ts, const float* vol,
                                 const float* bbox_min, const float* bbox_scale, const float* hann_w, const void* nr_packed,
                                 const void* cnl_packed, const float* bgcolor, int mode, float cull_eps, int64_t N, int S,
                                 int B, int G, int64_t chunk, void* workspace, size_t workspace_bytes, float* rgb,
                                 float* alpha, float* depth, float* weights_on_rays, float* rgb_on_rays, float* cnl_xyz,
                                 float* cnl_rgb, float* cnl_weight, float* xyz_on_rays, float* bmw, float* offsets,
                                 int* live_counts, void* side_stream, void* const* events, void* const* mlp_events,
                                 void* stream);

/* =============================== training (backward) ===============================
 * The reference trains through torch.autograd over the ops above (trainer.py:206-220).
 * Here: the forward runs the *_fwd_train variants (either arithmetic mode) which also save the
 * positional encodings, the post-ReLU activation matrices and their sign masks; the dX chain of
 * each MLP is one register-resident kernel (hnrf_*_bwd), the weight gradients come from
 * hnrf_mlp_dw, and the stages around the MLPs have the kernels below. */

/* pe_out [P,63] (columns in fourier.py order), acts [8][P][256] post-ReLU outputs of
 * pts_linears.{0..14}, relu_bits [8][P][8] uint32 (16-byte aligned): the sign masks of acts in the
 * register order of hnrf_canonical_bwd (opaque to the caller). */
int hnrf_canonical_fwd_train(const float* xyz, const void* packed, int mode, int64_t P,
                             float* raw, float* pe_out, float* acts, uint32_t* relu_bits, void* stream);
/* pe_out [P,36] (hannw_fourier.py order, window weights applied), acts [6][P][128],
 * relu_bits [6][P][4] uint32.
 * Both entry points write EVERY element of their outputs that a later kernel reads, whatever the buffers held before
 * (nothing is accumulated into, nothing needs to be cleared): rows 0 .. P-1 of raw / xyz / offsets, pe_out, acts and
 * relu_bits, and in HNRF_MLP_F16X3_H also
 *   - the padding columns of pe_out (63 of the canonical, 36..63 of the non-rigid matrix): zeros;
 *   - the padding rows P .. ceil(P / 128) * 128 - 1 of every blocked acts layer: a copy of row P-1 (finite values; the
 *     weight-gradient kernel multiplies them by the zero rows of dZ).
 * The non-rigid forward runs eight waves per workgroup when P is a multiple of 256 and four otherwise; the two forms
 * return the same bits for the same sample. */
int hnrf_nonrigid_fwd_train(const float* x_skel, const float* hann_w, const void* packed,
                            int mode, int64_t P, float* xyz, float* offsets,
                            float* pe_out, float* acts, uint32_t* relu_bits, void* stream);

/* Backward of hnrf_composite_fwd w.r.t. raw and fg_mask (autograd of network.py:355-379).
 *  g_rgb [R,3]; g_alpha, g_depth [R] or NULL.  Outputs d_raw [R,S,4], d_mask [R,S]. */
int hnrf_composite_bwd(const float* raw, const float* fg_mask, const float* z_vals,
                       const float* rays_d, const float* bgcolor,
                       const float* g_rgb, const float* g_alpha, const float* g_depth,
                       int64_t R, int S, float* d_raw, float* d_mask, void* stream);

/* Backward of the positional encodings w.r.t. the position (fourier.py / hannw_fourier.py).
 *  g [P, 3*include_input + 6*n_bands]; hann_w [n_bands] or NULL; dx [P,3] written or
 *  accumulated into. */
int hnrf_pe_bwd(const float* x, const float* g, const float* hann_w, int64_t P, int n_bands,
                int include_input, int accumulate, float* dx, void* stream);

/* Backward of hnrf_sample_warp_fwd w.r.t. the weight volume and the motion bases
 * (autograd of network.py:392-444, including grid_sample's gradient w.r.t. the grid).
 *  z_vals, x_skel, fg_mask: outputs of the forward; g_x_skel [R,S,3], g_mask [R,S].
 *  Outputs (overwritten): d_vol [B,G,G,G], d_Rs [B,3,3], d_Ts [B,3]. */
int hnrf_sample_warp_bwd(const float* rays_o, const float* rays_d, const float* z_vals,
                         const float* motion_Rs, const float* motion_Ts, const float* vol,
                         const float* bbox_min, const float* bbox_scale,
                         const float* x_skel, const float* fg_mask,
                         const float* g_x_skel, const float* g_mask,
                         int64_t R, int S, int B, int G,
                         float* d_vol, float* d_Rs, float* d_Ts, void* stream);

/* Per-frame kinematics: MotionBasisComputer.forward (core/utils/network_util.py:125-156) and its backward as one
 * single-wave kernel each (in PyTorch: 23 dependent 4x4 matmuls, a batched inverse and their autograd twins).
 *  dst_Rs [24,3,3], dst_Ts [24,3], cnl_gtfms [24,4,4] -> Rs [24,3,3], Ts [24,3] = (cnl_gtfms_i A_i^-1)[:3,:3 | :3,3],
 *  A_i = A_parent(i) [R_i | T_i] along the SMPL tree; fp64 internally.  saved (nullable): hnrf_motion_basis_saved_bytes()
 *  bytes, 8-byte aligned, for the backward.  B must be 24.  A saved that is not 8-byte aligned is HNRF_E_ARG, another B
 *  HNRF_E_UNSUPPORTED, in all four entries; nothing is written when a call is refused.
 *  bwd: g_Rs, g_Ts (gradients at the outputs) -> d_dst_Rs [24,3,3], d_dst_Ts [24,3]. */
size_t hnrf_motion_basis_saved_bytes(void);
int hnrf_motion_basis_fwd(const float* dst_Rs, const float* dst_Ts, const float* cnl_gtfms, int B, float* Rs, float* Ts,
                          void* saved, void* stream);
int hnrf_motion_basis_bwd(const float* g_Rs, const float* g_Ts, const float* dst_Rs, const float* dst_Ts,
                          const float* cnl_gtfms, int B, const void* saved, float* d_dst_Rs, float* d_dst_Ts, void* stream);
/* The same with the pose refinement in front folded in (BodyPoseRefiner's Rodrigues step, core/utils/network_util.py:57-83,
 * and the correction of core/nets/human_nerf/network.py:677-688): dst_Rs[i] <- dst_Rs[i] Rodrigues(rvec[i-1]) for the 23
 * non-root bones, theta = sqrt(1e-5 + |r|^2).  rvec [23,3] = the pose MLP's output.  bwd also returns d_rvec [23,3]
 * (d_dst_Rs is the gradient at the UNrefined rotations). */
int hnrf_refined_motion_basis_fwd(const float* rvec, const float* dst_Rs, const float* dst_Ts, const float* cnl_gtfms, int B,
                                  float* Rs, float* Ts, void* saved, void* stream);
int hnrf_refined_motion_basis_bwd(const float* g_Rs, const float* g_Ts, const float* rvec, const float* dst_Rs,
                                  const float* dst_Ts, const float* cnl_gtfms, int B, const void* saved, float* d_rvec,
                                  float* d_dst_Rs, float* d_dst_Ts, void* stream);

/* The pose refiner's MLP on one pose vector (BodyPoseRefiner.block_mlps, core/nets/human_nerf/pose_decoders/
 * mlp_delta_body_pose.py:14-41: Linear + ReLU x mlp_depth, then Linear) and its backward: one small launch per layer
 * each way (PyTorch: ~30 launches per training step for 0.5 MFLOP).
 *  W, b: HOST arrays of `layers` device pointers to the nn.Linear weights (out, in) row-major / biases; dims: HOST array
 *  of layers + 1 widths (dims[0] inputs, dims[l + 1] outputs of layer l), every width <= 256, layers <= 9.
 *  saved: hnrf_pose_mlp_saved_bytes(layers) bytes of device memory: the forward leaves the hidden activations there,
 *  the backward reads them and uses the rest as scratch.
 *  fwd: x [dims[0]] -> out [dims[layers]].
 *  bwd: g_out [dims[layers]] -> dW[l] (out, in), db[l] (HOST arrays of device pointers); d_x_parts (nullable): [8][256]
 *  floats whose first ceil(dims[1] / 32) rows sum to d_x (columns < dims[0]); the other rows and the columns from
 *  dims[0] on are not written. */
size_t hnrf_pose_mlp_saved_bytes(int layers);
int hnrf_pose_mlp_fwd(const float* x, const float* const* W, const float* const* b, const int* dims, int layers, float* out,
                      float* saved, void* stream);
int hnrf_pose_mlp_bwd(const float* g_out, const float* x, const float* const* W, const float* const* b, const int* dims,
                      int layers, float* saved, float* const* dW, float* const* db, float* d_x_parts, void* stream);

/* Weight / bias gradient of one nn.Linear inside the two MLPs (autograd of the Linear layers of
 * canonical_mlps/mlp_rgb_sigma.py and non_rigid_motion_mlps/mlp_offset.py under trainer.py:139-170):
 *   dW[o][i] = sum_s dZ[s][o] X[s][i]  for o < n_out, i < n_in;   db[o] = sum_s dZ[s][o]  (db may be NULL).
 *  dZ [P, ldz >= n_out], X [P, ldx >= n_in] row-major fp32; dW written with row stride ldw (so the two
 *  column blocks of a skip layer's weight are two calls).  Built shapes: n_out 128 | 256 with
 *  n_in 128 | 256 (X 16-byte aligned, ldx % 4 == 0) or n_in <= 64 (any ldx: the PE matrices);
 *  n_out <= 4 (the sigma/rgb and offset heads) with n_in 128 | 256.
 *  mode HNRF_MLP_F32: fp32 MFMA.  HNRF_MLP_F16X3: split-f16 MFMA at fp32-class accuracy for the matrix-shaped
 *  layers (n_out, n_in in {128, 256}; other shapes silently use the fp32 kernels); needs dz_amax = n_amax device
 *  floats whose maximum is >= max |dZ| (one row of hnrf_*_bwd's dz_amax), and |X| <= 65504.  Deterministic (fixed-order slice reduction).
 *  workspace: hnrf_mlp_dw_workspace_bytes (covers both modes), 256-byte aligned like every other workspace (HNRF_E_ARG
 *  otherwise; a smaller one is HNRF_E_WORKSPACE); nothing is written when the call is refused.  Every slice partial the
 *  reduction reads is written by the same call: the workspace needs no clearing between calls of different shapes.
 *  Only the n_in columns of each of the n_out rows of dW are written: the other columns of a wider matrix keep what
 *  they held. */
size_t hnrf_mlp_dw_workspace_bytes(int64_t P, int n_out, int n_in);
int hnrf_mlp_dw(const float* dZ, int64_t ldz, const float* X, int64_t ldx, int64_t P, int n_out, int n_in,
                int mode, const float* dz_amax, int n_amax, float* dW, int64_t ldw, float* db, void* workspace,
                size_t workspace_bytes, void* stream);

/* The same weight / bias gradient from HALF-PRECISION operands (training with the activations and dZ stored as
 * f16: half the HBM traffic of the step's two largest buffers).  dZ [P, ldz] and X [P, ldx] are row-major f16
 * (16-byte aligned, strides multiples of 8 halves, X rows padded with zeros to 64 / 128 / 256 columns); dZ may carry a
 * power-of-two scale: dz_scale (nullable device scalar) is divided out of dW and db.  One f16 MFMA per product,
 * fp32 accumulation over the samples; both operands reach the matrix pipe through gfx950's transposed LDS read
 * (ds_read_b64_tr_b16).  Each operand is rounded to 11 bits, unbiased: the relative error of a sum over N samples is
 * ~2^-12 / sqrt(N).  n_out <= 4 (heads): dZ is the fp32 [P, n_out] gradient at the head output, X the f16 activations.
 * Same shapes, workspace rules (hnrf_mlp_dw_h_workspace_bytes, 256-byte aligned: HNRF_E_ARG otherwise; a smaller one is
 * HNRF_E_WORKSPACE; nothing is written when the call is refused) and determinism as hnrf_mlp_dw.
 * layout: 0 = both matrices row-major; HNRF_DWH_DZ_BLOCKED / HNRF_DWH_X_BLOCKED = the matrix is in the BLOCKED layout
 * the HNRF_MLP_F16X3_H training kernels write (32-sample blocks of [32-feature tile][4 groups][2][32 samples][4 halves],
 * layers padded to a multiple of 128 samples; row strides are ignored for it).  Built: none, dZ only, both. */
#define HNRF_DWH_DZ_BLOCKED 1
#define HNRF_DWH_X_BLOCKED  2
size_t hnrf_mlp_dw_h_workspace_bytes(int64_t P, int n_out, int n_in);
int hnrf_mlp_dw_h(const void* dZ, int64_t ldz, const void* X, int64_t ldx, int64_t P, int n_out, int n_in, int layout,
                  const float* dz_scale, float* dW, int64_t ldw, float* db, void* workspace, size_t workspace_bytes,
                  void* stream);

/* Backward through all layers of one MLP (the dX chain of autograd over mlp_rgb_sigma.py / mlp_offset.py),
 * register-resident like the forward, with the backward of the positional encoding fused.
 *  *_bwd_pack: transposed weight image from the same nn.Linear weights hnrf_*_pack takes (re-pack after
 *  every parameter update); it writes every one of the *_bwd_packed_bytes(mode) bytes (16-byte aligned), so that two
 *  images of the same weights compare equal byte for byte.
 *  canonical: xyz [P,3], d_raw [P,4] (16-byte aligned), relu_bits [8][P][8] from hnrf_canonical_fwd_train ->
 *    dZ [8][P][256] (gradient at every hidden layer's pre-activation: the dZ operand of hnrf_mlp_dw) and
 *    d_xyz [P,3].
 *  non-rigid: x_skel [P,3], hann_w [6], d_xyz [P,3], relu_bits [6][P][4] from hnrf_nonrigid_fwd_train ->
 *    dZ [6][P][128] and d_x_skel [P,3] = d_xyz + J_offset^T d_xyz  (xyz = x_skel + offset, network.py:518-530). */
size_t hnrf_canonical_bwd_packed_bytes(int mode);
size_t hnrf_nonrigid_bwd_packed_bytes(int mode);
int hnrf_canonical_bwd_pack(const float* const* weights, int mode, void* packed, void* stream);
int hnrf_nonrigid_bwd_pack(const float* const* weights, int mode, void* packed, void* stream);
/* dz_amax (nullable): [L][HNRF_AMAX_SLOTS] floats; max over row l bounds |dZ_l| (the scale input of
 * hnrf_mlp_dw in HNRF_MLP_F16X3 mode). */
#define HNRF_AMAX_SLOTS 64
/* mode HNRF_MLP_F16X3 / HNRF_MLP_F16X3_H: the chain on the split-f16 matrix pipe; d_raw_amax / d_xyz_amax = device
 * scalar >= the largest magnitude of the incoming gradient, ignored in HNRF_MLP_F32.  The amax contract:
 *   - it only sets a power-of-two scale (the incoming gradient is brought to |g| < 4), so the results do not depend on
 *     the size of the gradient: g x 2^-24 and g x 2^10 give the same relative accuracy as g;
 *   - it need not be tight.  Every factor of two of slack costs one bit of the range below the largest value: of the
 *     22-bit split operands' 2^-14 floor in HNRF_MLP_F16X3 (harmless), of the f16 dZ stored by HNRF_MLP_F16X3_H (small
 *     dZ reach f16 subnormals earlier).  A bound 1000 x the true maximum (10 bits) keeps dW / db within the 1e-3 the
 *     f16 operands are specified to; keep it within that factor;
 *   - 0 (an all-zero incoming gradient) is valid: the scale is then 4, every dZ, d_xyz and weight gradient comes out
 *     exactly 0, d_x_skel = d_xyz bit for bit, and the per-layer scales returned in HNRF_MLP_F16X3_H are finite and > 0;
 *   - inf or NaN (an overflowed loss; the caller's maximum of a gradient with a non-finite element) makes the scale NaN:
 *     d_xyz / d_x_skel, dZ and every weight gradient computed from them by hnrf_mlp_dw / hnrf_mlp_dw_h contain NaN (in
 *     HNRF_MLP_F16X3 the maxima in dz_amax are NaN, in HNRF_MLP_F16X3_H the scales are), so that a finite check of
 *     ANY gradient tensor sees it.  Units whose ReLU is dead are masked by select and may stay 0.
 * The padding contract: rows 0 .. P-1 of dZ and d_xyz / d_x_skel and all of dz_amax are written whatever the buffers
 * held before; in HNRF_MLP_F16X3_H the padding rows P .. ceil(P / 128) * 128 - 1 of every blocked dZ layer are written
 * with ZEROS (hnrf_mlp_dw_h reads whole 128-sample blocks).  Nothing is read before it is written.  P == 0 returns
 * HNRF_OK without a launch: nothing is written, dz_amax included. */
int hnrf_canonical_bwd(const float* xyz, const float* d_raw, const uint32_t* relu_bits, const void* packed,
                       int mode, const float* d_raw_amax, int64_t P, float* dZ, float* d_xyz, float* dz_amax,
                       void* stream);
int hnrf_nonrigid_bwd(const float* x_skel, const float* hann_w, const float* d_xyz, const uint32_t* relu_bits,
                      const void* packed, int mode, const float* d_xyz_amax, int64_t P, float* dZ, float* d_x_skel,
                      float* dz_amax, void* stream);

/* =============================== in front of the path ===============================
 * Ray generation + bbox intersection + order-preserving compaction (get_rays_from_KRT,
 * core/utils/camera_util.py:132-159; rays_intersect_3d_bbox, camera_util.py:162-208; called per frame at
 * core/data/human_nerf/freeview.py:220-230 and its siblings).
 *  Kinv [3,3] = inverse intrinsics, R [3,3], T [3] = extrinsics, bbox_min / bbox_max [3] (unpadded; the 1 cm pad
 *  is applied inside), all float32 device pointers.  Outputs, in pixel order: ray_mask [H*W] (1 = the ray crosses
 *  the box), and for the *count kept rays rays_o / rays_d [count,3] (direction un-normalised, components clamped
 *  to 1e-5 like the reference), near / far [count].  Size the ray buffers for H*W; their entries from *count on
 *  are not written.  workspace: hnrf_gen_rays_workspace_bytes(H, W) bytes, 256-byte aligned like every other workspace
 *  (HNRF_E_ARG otherwise; a smaller one is HNRF_E_WORKSPACE); nothing is written when the call is refused. */
size_t hnrf_gen_rays_workspace_bytes(int H, int W);
int hnrf_gen_rays(const float* Kinv, const float* R, const float* T, const float* bbox_min, const float* bbox_max,
                  int H, int W, float* rays_o, float* rays_d, float* near, float* far, uint8_t* ray_mask,
                  int* count, void* workspace, size_t workspace_bytes, void* stream);

/* ---- image pre-processing of Dataset.load_image (core/data/human_nerf/train.py:351-417, freeview.py:137-166) ----
 * The reference decodes a frame's image and mask PNGs and runs cv2.undistort on both (train.py:366-371: every
 * prepared ZJU-MoCap camera has `distortions`, tools/prepare_zju_mocap/prepare_dataset.py:172-176), composites
 * mask/255 * image + (1 - mask/255) * bgcolor in float64 (train.py:406) and, for resize_img_scale != 1 (0.5 in
 * every 387 / wild yaml), cv2.resize with INTER_LANCZOS4 (image) and INTER_LINEAR (mask) (train.py:408-417).
 * humannerf_amd/imageproc.py is the host statement of the same OpenCV functions (cv2 is not importable: parity with
 * OpenCV's binaries is unpinned; the two statements agree bit for bit).
 *
 * hnrf_undistort_image: src / dst uint8 [H,W,C] (C <= 4, not in place).  cam = {fx, fy, u0, v0, k1, k2, p1, p2, k3}
 *  and ir = [n_stripes][9] row-major inverses of K with its principal point moved to the stripe's first row
 *  (cv2.undistort works in stripes of stripe_rows = min(max(1, 4096 / W), H) rows), both float64 DEVICE arrays.
 *  Fixed-point map (1/32 pixel), bilinear taps with remap's 15-bit weights, constant 0 outside the image. */
int hnrf_undistort_image(const uint8_t* src, int H, int W, int C, const double* cam, const double* ir, int n_stripes,
                         int stripe_rows, uint8_t* dst, void* stream);
/* hnrf_composite_windows: orig / alpha uint8 [Hs,Ws,3] (alpha in 0..255), bgcolor float32 [3] in 0..255 ->
 *  out float32 [n_win, ph, pw, 3] = composite / 255 for the windows whose top-left DESTINATION pixels are
 *  win_xy[n_win][2] = (x0, y0) (int32, device; windows must lie inside [Hd, Wd]).  resize = 0: destination grid =
 *  source grid (Hd == Hs, Wd == Ws, tables ignored).  resize = 1: INTER_LANCZOS4 from the coefficient tables of
 *  hal::resize's setup loop -- xofs [Wd] / yofs [Hd] int32 (index of the tap left of the sample point), xw [Wd][8] /
 *  yw [Hd][8] float32 -- horizontal then vertical pass over the float64 composite, taps clamped to the border.
 *  A training item's 6 windows of 32x32 (cfg.patch) or a whole image (one window) alike. */
int hnrf_composite_windows(const uint8_t* orig, const uint8_t* alpha, int Hs, int Ws, const float* bgcolor, int resize,
                           const int* xofs, const float* xw, const int* yofs, const float* yw, int Hd, int Wd,
                           const int* win_xy, int n_win, int ph, int pw, float* out, void* stream);
/* hnrf_resize_mask: channel `channel` of the uint8 mask [Hs,Ws,3], divided by 255, through cv2.resize INTER_LINEAR ->
 *  out float32 [Hd,Wd] (the dataset only asks whether it is > 0: train.py:620-631).  mode 1: two-tap tables
 *  (xw [Wd][2], yw [Hd][2]); mode 2: the 2x2 box mean hal::resize substitutes at scale exactly 1/2. */
int hnrf_resize_mask(const uint8_t* alpha, int Hs, int Ws, int channel, int mode, const int* xofs, const float* xw,
                     const int* yofs, const float* yw, int Hd, int Wd, float* out, void* stream);

/* ---- weight-volume decoder glue (MotionWeightVolumeDecoder, mweight_vol_decoders/deconv_vol_decoder.py:25-33;
 * ConvDecoder3D, core/utils/network_util.py:12-50) ----
 * hnrf_deconv_fold: the scatter half of nn.ConvTranspose3d(kernel 4, stride 2, padding 1) on a batch-1 volume.
 *  col [D*H*W, cout*64] = x^T W (one GEMM on the weight's native (cin, cout, 4,4,4) layout, done by the caller's BLAS),
 *  bias [cout] or NULL -> out [cout, 2D, 2H, 2W]: out[co, 2d-1+kd, 2h-1+kh, 2w-1+kw] += col[(d,h,w), co*64 + kd*16+kh*4+kw],
 *  written as a gather per output voxel (deterministic, no atomics). */
int hnrf_deconv_fold(const float* col, const float* bias, int cout, int D, int H, int W, float* out, void* stream);

/* ---- mesh extraction of the canonical body (no counterpart in the reference; humannerf_amd/mesh.py) ----
 * hnrf_density_grid: the canonical density on an N^3 lattice (8 <= N <= 512) over [bbox_min, bbox_max] [3] each,
 *  indexed [z][y][x], x fastest; point (x,y,z) at bbox_min + (float)i * step, step = (bbox_max - bbox_min) / (N - 1),
 *  each operation rounded on its own.  density [N^3] = relu(sigma) * fg: sigma = channel 3 of the canonical MLP
 *  (cnl_packed, mode as hnrf_canonical_fwd), fg = sum over the B bone channels of vol [>= B, G, G, G] sampled like
 *  K1 (bbox_min / bbox_scale [3], align_corners, zero padding) under the identity motion.  Nullable: sigma [N^3],
 *  fg [N^3].  Runs in chunks of hnrf_canonical_fwd through `workspace` (hnrf_density_grid_workspace_bytes(N),
 *  256-byte aligned); every chunk is guarded (HNRF_STATUS_F16_RANGE in cnl_packed's status word, mode f16x3).
 * hnrf_mesh_count / hnrf_mesh_emit: marching tetrahedra (Kuhn decomposition: 6 tetrahedra per cell around its main
 *  diagonal) of density [N^3] at `level` (inside: density > level).  Each lattice point owns its edges to the +x, +y,
 *  +z, +xy, +xz, +yz, +xyz neighbour (slots 0..6); one vertex per edge that crosses the level, at pa + t (pb - pa),
 *  t = (level - da) / (db - da), a = the owning point; vertices ordered by (point, slot), triangles by (cell,
 *  tetrahedron 0..5, triangle 0..1), wound counter-clockwise seen from outside ((v1 - v0) x (v2 - v0) points toward
 *  lower density).  Watertight and edge-manifold except where the surface meets the lattice boundary: it stays open
 *  there.  Bit-reproducible (integer block scans, no atomics).
 *  hnrf_mesh_count writes counts [2] = {V, F} (int64, device) and fills `workspace` (hnrf_mesh_workspace_bytes(N),
 *  256-byte aligned); the caller reads the counts, allocates verts [V,3] fp32 and faces [F,3] int32 (vertex ids,
 *  V < 2^31) and passes the same density, level and workspace to hnrf_mesh_emit (bbox_max > bbox_min on every axis,
 *  or the winding flips).  Writes past V / F are dropped. */
size_t hnrf_density_grid_workspace_bytes(int N);
int hnrf_density_grid(const void* cnl_packed, int mode, const float* vol, int B, int G, const float* bbox_min,
                      const float* bbox_max, const float* bbox_scale, int N, void* workspace, size_t workspace_bytes,
                      float* density, float* sigma, float* fg, void* stream);
size_t hnrf_mesh_workspace_bytes(int N);
int hnrf_mesh_count(const float* density, int N, float level, void* workspace, size_t workspace_bytes, int64_t* counts,
                    void* stream);
int hnrf_mesh_emit(const float* density, int N, float level, const float* bbox_min, const float* bbox_max,
                   const void* workspace, size_t workspace_bytes, int64_t V, int64_t F, float* verts, int* faces,
                   void* stream);
/* hnrf_forward_skin: canonical vertices verts [V,3] -> posed out [V,3],
 *  x_o = sum_b w_b(x_c) A_b^-1(x_c) / max(sum_b w_b, 1e-4), A_b(x) = R_b x + T_b the frame's motion basis
 *  (motion_Rs [B,3,3], motion_Ts [B,3], B <= 128), w_b = the trilinear weight of bone b of vol at the canonical
 *  vertex (bbox_min / bbox_scale as K1).  The forward counterpart of K1's inverse warp; the non-rigid offsets are not
 *  inverted.  vol [>= B,G,G,G]: the first B channels are read.  V >= 0 (V = 0: nothing is launched and the pointers are
 *  not looked at). */
int hnrf_forward_skin(const float* verts, int64_t V, const float* motion_Rs, const float* motion_Ts, const float* vol,
                      int B, int G, const float* bbox_min, const float* bbox_scale, float* out, void* stream);

/* ---- baked canonical grid (no counterpart in the reference; humannerf_amd/baked.py) ----
 * In the configuration this library builds (no view direction, no pose colour, no condition code) the canonical MLP is
 * a pure function of the canonical position: raw = f(xyz), the same for every frame, pose and camera until the weights
 * change.  It can be tabulated once per checkpoint and interpolated afterwards -- an opt-in APPROXIMATION like
 * cull_eps / term_eps (not the reference arithmetic): K1, K2, K4, culling and all 11 outputs stay exact, only raw
 * comes from interpolation.
 * grid [N][N][N][4] f16, indexed [z][y][x][c], c = (r, g, b, sigma) PRE-activation, 8 bytes per lattice point
 *  (hnrf_baked_grid_bytes(N); 8-byte aligned), 8 <= N <= 512.  Lattice exactly as hnrf_density_grid's: point i on an
 *  axis at bbox_min + (float)i * step, step = (bbox_max - bbox_min) / (N - 1), each operation rounded on its own.
 * hnrf_bake_canonical: value = hnrf_canonical_fwd at the lattice point in `mode`, converted to f16 with round to
 *  nearest even; values beyond +-65504 (infinities included) are stored as +-65504 and counted into *saturated
 *  (nullable device counter, ADDED to: the caller zeroes it); NaN stays NaN.  Runs in chunks through `workspace`
 *  (hnrf_bake_canonical_workspace_bytes(N), 256-byte aligned); every chunk is range-guarded (HNRF_STATUS_F16_RANGE in
 *  cnl_packed's status word, mode f16x3).
 * hnrf_baked_sample: xyz [P,3] -> raw [P,4] fp32 (16-byte aligned), what hnrf_canonical_fwd writes.  Per axis, with
 *  n = N - 1: inv_step = (float)n / (bbox_max - bbox_min); u = (x - bbox_min) * inv_step; u = min(max(u, 0), n) --
 *  border replicate: points outside the box sample the clamped point, a NaN coordinate samples index 0 --;
 *  i0 = min((int)floor(u), n - 1); t = u - (float)i0.  Blend in fp32, every channel on its own, every operation
 *  rounded on its own (no fma), a + t * (b - a) first along x (4 times), then along y (twice), then along z.
 *  humannerf_amd/baked.py:sample_host restates it in numpy float32, bit for bit.
 * hnrf_baked_sample_sparse: only the samples idx[0 .. *count) are read and written (semantics of
 *  hnrf_canonical_fwd_sparse). */
size_t hnrf_baked_grid_bytes(int N);
size_t hnrf_bake_canonical_workspace_bytes(int N);
int hnrf_bake_canonical(const void* cnl_packed, int mode, const float* bbox_min, const float* bbox_max, int N,
                        void* workspace, size_t workspace_bytes, void* grid, unsigned* saturated, void* stream);
int hnrf_baked_sample(const float* xyz, const void* grid, int N, const float* bbox_min, const float* bbox_max, int64_t P,
                      float* raw, void* stream);
int hnrf_baked_sample_sparse(const float* xyz, const void* grid, int N, const float* bbox_min, const float* bbox_max,
                             int64_t P, const int* idx, const int* count, float* raw, void* stream);
/* hnrf_render_rays_fwd / hnrf_render_frame_fwd with the grid sampler in the canonical MLP's place: the arguments of
 * those entries with cnl_packed replaced by grid, grid_N, grid_bbox_min, grid_bbox_max (the box the grid was baked
 * over: device pointers [3]).  Lean and 11-output forms, cull_eps, the side stream and the event pairs (recorded
 * around the sampler launch) as there; `mode` is the non-rigid MLP's, whose image is still guarded.  There is no
 * canonical status word in this form, and no early-termination form. */
int hnrf_render_rays_baked_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                               const float* t_rand, const float* motion_Rs, const float* motion_Ts, const float* vol,
                               const float* bbox_min, const float* bbox_scale, const float* hann_w, const void* nr_packed,
                               const void* grid, int grid_N, const float* grid_bbox_min, const float* grid_bbox_max,
                               const float* bgcolor, int mode, float cull_eps, int64_t R, int S, int B, int G,
                               void* workspace, size_t workspace_bytes, float* rgb, float* alpha, float* depth,
                               void* ev_mlp_start, void* ev_mlp_stop, void* stream);
int hnrf_render_frame_baked_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                const float* t_rand, const float* motion_Rs, const float* motion_Ts, const float* vol,
                                const float* bbox_min, const float* bbox_scale, const float* hann_w, const void* nr_packed,
                                const void* grid, int grid_N, const float* grid_bbox_min, const float* grid_bbox_max,
                                const float* bgcolor, int mode, float cull_eps, int64_t N, int S, int B, int G,
                                int64_t chunk, void* workspace, size_t workspace_bytes, float* rgb, float* alpha,
                                float* depth, float* weights_on_rays, float* rgb_on_rays, float* cnl_xyz, float* cnl_rgb,
                                float* cnl_weight, float* xyz_on_rays, float* bmw, float* offsets, void* side_stream,
                                void* const* events, void* const* mlp_events, void* stream);

/* ---- baked non-rigid offset field (no counterpart in the reference; humannerf_amd/baked.py) ----
 * Within one frame the condition code and the Hann window weights are constants, so K2's offset is a function of the
 * three coordinates of x_skel alone: offset = g(x_skel).  It can be tabulated once per FRAME and interpolated -- an
 * opt-in APPROXIMATION on the lines of the baked canonical grid, and only together with it.
 * off_grid [M][M][M][4] f16, indexed [z][y][x][c], c = (dx, dy, dz, +0.0), 8 bytes per lattice point
 *  (hnrf_baked_grid_bytes(M); 8-byte aligned), 8 <= M <= 512; the lattice and the layout are the canonical grid's, so
 *  that one sampler serves both.
 * hnrf_bake_nonrigid: value = the `offsets` output of hnrf_nonrigid_fwd (nr_packed, hann_w, mode) at the lattice point,
 *  converted to f16 with round to nearest even; values beyond +-65504 (infinities included) are stored as +-65504 and
 *  counted into *saturated (nullable device counter, ADDED to); NaN stays NaN; the pad lane is +0.  Runs in chunks
 *  through `workspace` (hnrf_bake_nonrigid_workspace_bytes(M), 256-byte aligned); every chunk is range-guarded
 *  (HNRF_STATUS_F16_RANGE in nr_packed's status word, mode f16x3).
 * hnrf_baked_warp_sample: x_skel [P,3] -> raw [P,4] fp32 (16-byte aligned); nullable xyz [P,3], offsets [P,3].  With
 *  `sample` = hnrf_baked_sample's arithmetic and every operation rounded on its own:
 *      off = channels 0..2 of sample(off_grid, M, off_bbox) at x_skel
 *      xyz = x_skel + off          (one fp32 add per coordinate)
 *      raw = sample(grid, N, bbox) at xyz
 *  bit for bit the chain hnrf_baked_sample -> add -> hnrf_baked_sample, in one kernel without the 24 B / sample round
 *  trip of K2's output.  humannerf_amd/baked.py:warp_sample_host restates it in numpy float32.
 * hnrf_baked_warp_sample_sparse: only the samples idx[0 .. *count) are read and written (raw, xyz and offsets alike;
 *  semantics of hnrf_baked_sample_sparse). */
size_t hnrf_bake_nonrigid_workspace_bytes(int M);
int hnrf_bake_nonrigid(const void* nr_packed, const float* hann_w, int mode, const float* bbox_min, const float* bbox_max,
                       int M, void* workspace, size_t workspace_bytes, void* grid, unsigned* saturated, void* stream);
int hnrf_baked_warp_sample(const float* x_skel, const void* off_grid, int off_M, const float* off_bbox_min,
                           const float* off_bbox_max, const void* grid, int grid_N, const float* grid_bbox_min,
                           const float* grid_bbox_max, int64_t P, float* raw, float* xyz, float* offsets, void* stream);
int hnrf_baked_warp_sample_sparse(const float* x_skel, const void* off_grid, int off_M, const float* off_bbox_min,
                                  const float* off_bbox_max, const void* grid, int grid_N, const float* grid_bbox_min,
                                  const float* grid_bbox_max, int64_t P, const int* idx, const int* count, float* raw,
                                  float* xyz, float* offsets, void* stream);
/* hnrf_render_rays_baked_fwd / hnrf_render_frame_baked_fwd with the fused sampler above in the place of K2 and the grid
 * sampler: the arguments of those entries with hann_w, nr_packed replaced by off_grid, off_M, off_bbox_min,
 * off_bbox_max.  Lean and 11-output forms, cull_eps, the side stream and the event pairs (recorded around the fused
 * sampler's launch) as there.  In the 11-output form xyz_on_rays and offsets are the interpolated values actually used;
 * backward_motion_weights stays exact.  No MLP runs: `mode` is checked and otherwise unused, and there is no status
 * word in this form. */
int hnrf_render_rays_baked_nr_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                  const float* t_rand, const float* motion_Rs, const float* motion_Ts, const float* vol,
                                  const float* bbox_min, const float* bbox_scale, const void* off_grid, int off_M,
                                  const float* off_bbox_min, const float* off_bbox_max, const void* grid, int grid_N,
                                  const float* grid_bbox_min, const float* grid_bbox_max, const float* bgcolor, int mode,
                                  float cull_eps, int64_t R, int S, int B, int G, void* workspace, size_t workspace_bytes,
                                  float* rgb, float* alpha, float* depth, void* ev_mlp_start, void* ev_mlp_stop,
                                  void* stream);
int hnrf_render_frame_baked_nr_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                   const float* t_rand, const float* motion_Rs, const float* motion_Ts, const float* vol,
                                   const float* bbox_min, const float* bbox_scale, const void* off_grid, int off_M,
                                   const float* off_bbox_min, const float* off_bbox_max, const void* grid, int grid_N,
                                   const float* grid_bbox_min, const float* grid_bbox_max, const float* bgcolor, int mode,
                                   float cull_eps, int64_t N, int S, int B, int G, int64_t chunk, void* workspace,
                                   size_t workspace_bytes, float* rgb, float* alpha, float* depth, float* weights_on_rays,
                                   float* rgb_on_rays, float* cnl_xyz, float* cnl_rgb, float* cnl_weight,
                                   float* xyz_on_rays, float* bmw, float* offsets, void* side_stream,
                                   void* const* events, void* const* mlp_events, void* stream);

/* ---- rasteriser for vertex-coloured triangle meshes (no counterpart in the reference; humannerf_amd/raster.py) ----
 * hnrf_raster_mesh: verts [V,3] fp32 world positions, faces [F,3] int32, colors [V,3] fp32 (nullable when the shade
 *  is the normal), camera K [9], R [9] (row-major 3x3), T [3], bgcolor [3] (0..1): device pointers, nothing is read
 *  on the host.  Every float operation rounded on its own, sums associated left to right as written (raster.py
 *  restates all of it in numpy, bit for bit):
 *  - projection in fp32: xc_i = ((R_i0 x + R_i1 y) + R_i2 z) + T_i, p_i = (K_i0 xc_0 + K_i1 xc_1) + K_i2 xc_2,
 *    u = p_0 / p_2, v = p_1 / p_2, z = xc_2, w = 1 / z; pixel (i, j) is sampled at screen position (i, j) exactly;
 *  - positions snapped to 1/256 pixel, X = rint(256 u) (half to even); coverage is 64-bit integer arithmetic: with
 *    a = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0), s = sign(a), the edge values E0 = s cross(P2 - P1, S - P1),
 *    E1 = s cross(P0 - P2, S - P2), E2 = s cross(P1 - P0, S - P0) at S = (256 i, 256 j), cross(d, q) = d_x q_y - d_y q_x;
 *  - a triangle is dropped whole when an index is outside [0, V) (nothing is read there), when a vertex fails
 *    z >= z_near && |u| <= 16384 && |v| <= 16384 && w > 0 (NaN fails; no clipping), or when a = 0;
 *  - top-left fill rule in the triangle's own positive orientation (independent of the winding): inside iff for every
 *    edge E_k > 0, or E_k = 0 and the oriented edge vector d has d_y < 0 or (d_y = 0 and d_x > 0); triangles sharing an
 *    edge never both own a sample on it and never both miss it;
 *  - flags & HNRF_RASTER_CULL_MASK: NONE (two-sided) | BACK | FRONT; front-facing (the winding normal
 *    (v1 - v0) x (v2 - v0) faces the camera) is (a < 0) != (det(K R) < 0), the determinant in fp32 on the device;
 *  - inverse depth per sample in fp64: b_k = E_k / |a|, w = (w0 + b1 (w1 - w0)) + b2 (w2 - w0), rounded to fp32; the
 *    visible triangle has the largest w, among equal w the lowest index: key = bits(w) << 32 | 0xFFFFFFFF - index is
 *    folded into a 64-bit-per-pixel buffer with an atomic maximum, so the result does not depend on the order of
 *    processing and is bit-reproducible;
 *  - outputs [H,W] (each nullable): tri_id int32 (-1 = background), depth = 1 / w (0 on background), alpha 1 / 0,
 *    rgb [H,W,3] = bgcolor on background, else q_k = b_k w_k, ((q0 c0 + q1 c1) + q2 c2) / ((q0 + q1) + q2) in fp64
 *    rounded to fp32 (perspective-correct), or with HNRF_RASTER_SHADE_NORMAL 0.5 + 0.5 n, n = R m, m = the normalised
 *    winding normal of the fp32 world positions in fp32 (0 when its length is 0 or not finite), not flipped toward
 *    the viewer.
 *  1 <= H, W <= 8192, V, F < 2^31, z_near > 0, known flags (HNRF_E_UNSUPPORTED otherwise; null pointers HNRF_E_ARG);
 *  V == 0 or F == 0 renders the background.  `workspace`: hnrf_raster_workspace_bytes(V, F, H, W), 256-byte aligned
 *  (0 for arguments out of range).  No allocation, no synchronisation. */
#define HNRF_RASTER_CULL_NONE    0
#define HNRF_RASTER_CULL_BACK    1
#define HNRF_RASTER_CULL_FRONT   2
#define HNRF_RASTER_CULL_MASK    3
#define HNRF_RASTER_SHADE_NORMAL 4
size_t hnrf_raster_workspace_bytes(int64_t V, int64_t F, int H, int W);
int hnrf_raster_mesh(const float* verts, int64_t V, const int* faces, int64_t F, const float* colors, const float* K,
                     const float* R, const float* T, const float* bgcolor, int H, int W, float z_near, int flags,
                     float* rgb, float* alpha, float* depth, int* tri_id, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---- LPIPS ---- the perceptual loss and metric LPIPS(net='vgg', version='0.1', lpips=True, layers=[0..4]) in eval mode
 * (third_parties/lpips/lpips.py:84-129, pretrained_networks.py:96-134, __init__.py:40-42; humannerf_amd/lpips.py).
 * The arithmetic, stated once:
 *  1. img0, img1: [N,H,W,3] fp32 in [-1, 1], NHWC; H, W >= 16 (HNRF_E_UNSUPPORTED below, before any launch).
 *  2. Scaling layer: s = (x - shift) / scale, shift = (-.030, -.088, -.188), scale = (.458, .448, .450), applied to
 *     in-range pixels as the first convolution loads them.  That convolution's zero padding is a zero of the SCALED
 *     image, so the shift is not folded into its bias (that would be wrong on every border pixel).
 *  3. Trunk: the 13 conv3x3 (pad 1, stride 1) + bias + ReLU layers of VGG16 features[0..29], layers 0..12 with
 *     (Cin, Cout) = (3,64) (64,64) | (64,128) (128,128) | (128,256) (256,256) (256,256) | (256,512) (512,512) (512,512) |
 *     (512,512) x 3; a 2x2 / stride-2 max-pool in floor mode (odd sizes drop the last row and column) at every `|`;
 *     taps after layers 1, 3, 6, 9, 12 with 64, 128, 256, 512, 512 channels.  Every convolution is an fp32 fma chain
 *     over k = tap * Cin + ci (v_mfma_f32_32x32x2_f32), in an order fixed by the layer and by H * W alone.
 *  4. Head: per tap f = x / (sqrt(sum_c x^2 + 1e-10) + 1e-10) for both images, d = (f0 - f1)^2,
 *     v_l = mean_{h,w} sum_c w_c d_c with the 1x1 head weights; the value is sum_l v_l, one per image pair.
 *  5. Backward: with respect to img0 only, the trunk is frozen.  conv backward-data = the same convolution on the
 *     second packed image (taps rotated 180 degrees, channel roles swapped), the incoming gradient masked by the saved
 *     output y > 0 on load; pool backward routes to the first maximum in row-major scan order (torch's CPU kernel); the
 *     chain through the scaling layer is / scale.
 *  6. Determinism: no floating-point atomics, every reduction in a fixed order; results are bit-identical from run to
 *     run, and pair n's value and gradient do not depend on the rest of the batch.
 * Activations are NHWC fp32, pointers 16-byte aligned; `packed` and `workspace` 256-byte aligned.
 *
 * hnrf_lpips_pack: w[13] / b[13] / lin[5] are HOST arrays of device pointers to the (Cout,Cin,3,3) weights, (Cout)
 *  biases and (C) head weights; `packed`: hnrf_lpips_packed_bytes() bytes.  Holds the forward image [Cout][9 Cin]
 *  (layer 0: K = 27 padded to 32), the backward-data image [Cin][9 Cout] (layer 0: 3 rows padded to 32), biases, heads.
 * hnrf_conv3x3_fwd: y [N,H,W,Cout] = relu(conv(x [N,H,W,Cin]) + bias) of trunk layer `layer`; scale_input (layer 0
 *  only) applies the scaling layer on load.  Any H, W >= 1.
 * hnrf_conv3x3_bwd_data: dx [N,H,W,Cin] from dy [N,H,W,Cout]; y_saved (nullable, dy's shape): dy counts only where
 *  y_saved > 0; unscale_output (layer 0 only): dx / scale.
 * hnrf_maxpool2_fwd / _bwd: x [N,H,W,C] -> y [N,H/2,W/2,C]; dx [N,H,W,C] from x and dy (every element written).  C % 4 == 0.
 * hnrf_lpips_head_fwd: f [2N,P,C] (maps of the N first images, then of the N second ones), w [C], C in {64,128,256,512};
 *  pix_ws [N P] scratch; out[n] = (accumulate ? out[n] : 0) + v[n]; layer_val (nullable) [N] = v.
 * hnrf_lpips_head_bwd: dx [N,P,C] (+)= grad_out[n] dv[n] / dx0.
 * hnrf_lpips_fwd: out [N]; per_layer (nullable) [5][N] the true per-tap values (the reference's retPerLayer list is
 *  aliased: `val = res[0]; val += res[l]` makes res[0] the total).  Both image sets run as one batch of 2N through every
 *  launch.  want_grad != 0 keeps the 13 activations in `workspace` for hnrf_lpips_bwd, which must get the same N, H, W
 *  and the untouched workspace; want_grad == 0 needs two buffers only.  hnrf_lpips_workspace_bytes: 0 for sizes refused.
 * hnrf_lpips_bwd: d_img0 [N,H,W,3] = sum_n grad_out[n] d value[n] / d img0.
 * No allocation, no synchronisation; null pointers HNRF_E_ARG, sizes / layers not built HNRF_E_UNSUPPORTED. */
size_t hnrf_lpips_packed_bytes(void);
int hnrf_lpips_pack(const float* const* w, const float* const* b, const float* const* lin, void* packed, void* stream);
int hnrf_conv3x3_fwd(const float* x, const void* packed, int layer, int N, int H, int W, int scale_input, float* y,
                     void* stream);
int hnrf_conv3x3_bwd_data(const float* dy, const float* y_saved, const void* packed, int layer, int N, int H, int W,
                          int unscale_output, float* dx, void* stream);
int hnrf_maxpool2_fwd(const float* x, int N, int H, int W, int C, float* y, void* stream);
int hnrf_maxpool2_bwd(const float* x, const float* dy, int N, int H, int W, int C, float* dx, void* stream);
int hnrf_lpips_head_fwd(const float* f, const float* w, int N, int64_t P, int C, float* pix_ws, float* out,
                        int accumulate, float* layer_val, void* stream);
int hnrf_lpips_head_bwd(const float* f, const float* w, const float* grad_out, int N, int64_t P, int C, float* dx,
                        int accumulate, void* stream);
size_t hnrf_lpips_workspace_bytes(int N, int H, int W, int want_grad);
int hnrf_lpips_fwd(const float* img0, const float* img1, const void* packed, int N, int H, int W, int want_grad,
                   void* workspace, size_t workspace_bytes, float* out, float* per_layer, void* stream);
int hnrf_lpips_bwd(const float* grad_out, const void* packed, int N, int H, int W, void* workspace,
                   size_t workspace_bytes, float* d_img0, void* stream);

/* ---- Image metrics ---- PSNR and SSIM of 8-bit image pairs that are on the device already: replaces, for uint8 images,
 * compute_psnr / compute_ssim as MetricsWriter.append calls them per frame on the host (metrics_util.py:78-106;
 * humannerf_amd/render.py psnr, ssim; the numpy statement of exactly this arithmetic is render.metrics_u8).
 *  pred, target [n_img,H,W,3] uint8; mask (nullable) [n_img,H,W] uint8, non-zero = inside; out [n_img][2] = psnr, ssim (fp64).
 *  - psnr = -10 log10(SSE / (255^2 count)), count = 3 H W or 3 nnz(mask), SSE an exact integer sum over the pixels
 *    inside; equal images give +inf, an empty mask NaN;
 *  - ssim: with a mask both images are cropped to the bounding box of its non-zero pixels (cv2.boundingRect); per
 *    channel a 7x7 uniform window at every position where it fits entirely, from exact int32 window sums of x, y, x^2,
 *    y^2, xy: ux = Sx / (49 255), uxx = Sxx / (49 255^2), vx = 49/48 (uxx - ux ux), C1 = (0.01 data_range)^2,
 *    C2 = (0.03 data_range)^2, s = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) in fp64 without
 *    contraction; the mean over the positions, then over the three channels.  A crop narrower than 7 in either
 *    direction (an empty mask included) gives NaN;
 *  - no atomics, every sum in a fixed order: bit-identical from run to run, and image n's values do not depend on
 *    the rest of the batch.
 * 1 <= n_img <= 65535, 1 <= H, W <= 8192, data_range > 0 (HNRF_E_UNSUPPORTED otherwise; null pointers HNRF_E_ARG;
 * hnrf_image_metrics_workspace_bytes: 0 for sizes refused).  `workspace` 256-byte aligned; the bounding boxes stay in it
 * between the four launches.  No allocation, no synchronisation, ordered on `stream`. */
size_t hnrf_image_metrics_workspace_bytes(int n_img, int H, int W);
int hnrf_image_metrics(const uint8_t* pred, const uint8_t* target, const uint8_t* mask, int n_img, int H, int W,
                       double data_range, void* workspace, size_t workspace_bytes, double* out, void* stream);

/* ---- Surface points and frame distance ---- one canonical surface point per ray (run.py:388-404, save_3d_together),
 * the brute-force nearest neighbour of two point clouds, and the batched, windowed frame x frame appearance distance of
 * tools/compute_distance*.py.  Additive to ABI version 13; contracts and declarations in hnrf_cloud.h. */
#include "hnrf_cloud.h"

/* ---- baseline JPEG encoding of 8-bit images on the device (the frames of a Motion-JPEG video).  Additive to ABI
 * version 13; contracts and declarations in hnrf_video.h. */
#include "hnrf_video.h"

/* ---- surface records split by body part (tools/segment.py): per-record part membership from a per-frame bitmap of
 * part masks, and the stable compaction per (part, frame).  Additive to ABI version 13; contracts and declarations in
 * hnrf_segment.h. */
#include "hnrf_segment.h"

/* ---- geometry maps of a rendered frame: the surface distance per ray, the pixel -> ray map, and the depth / normal /
 * shaded / non-rigid-offset panels (screen-space differences of the rendered surface distance).  Additive to ABI
 * version 13; contracts and declarations in hnrf_geometry.h. */
#include "hnrf_geometry.h"

/* ---- the multi-head canonical MLP (canonical_mlp.multihead, head_depth 1): pack, all heads of one trunk pass, and the
 * frame with per-head outputs.  Additive to ABI version 13; contracts and declarations in hnrf_heads.h. */
#include "hnrf_heads.h"

/* ---- the skinned glTF export: the K largest bone weights of every vertex, normalised, and the skinning sum a glTF
 * viewer performs with them.  Additive to ABI version 13; contracts and declarations in hnrf_skin.h. */
#include "hnrf_skin.h"

/* ---- every head of a multi-head canonical image with the shared evaluation of underflowing inputs: the n-plane
 * classification, stand-alone and fused into K1, and the frame entry that joins it with the all-heads K3.  Additive to
 * ABI version 13; contracts and declarations in hnrf_heads_shared.h. */
#include "hnrf_heads_shared.h"

/* ---- density-gradient normals: one observation-space normal per ray from the gradients the training kernels return,
 * the normal / shaded panels painted from them, and the normal of the gated density a mesh is cut from.  Additive to ABI
 * version 13; contracts and declarations in hnrf_normals.h. */
#include "hnrf_normals.h"

/* ---- training the multi-head canonical MLP: the all-heads epilogue on the activation-saving forward, the transposed
 * image with a 4 H-wide head stage, and the backward chain seeded with every head's gradient.  Additive to ABI version
 * 13; contracts and declarations in hnrf_heads_train.h. */
#include "hnrf_heads_train.h"

/* ---- view-dependent colour (canonical_mlp.view_dir): the per-ray colour bias the folded view branch leaves, K4 and K4'
 * with it, and the one frame entry that carries it through every inference path.  Additive to ABI version 13; contracts
 * and declarations in hnrf_view.h. */
#include "hnrf_view.h"

#ifdef __cplusplus
}
#endif
#endif /* HNRF_H */
