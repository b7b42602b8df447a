/* libhnrf -- the multi-head canonical MLP: every head of one trunk pass.  Included by hnrf.h (inside its extern "C");
 * additive to ABI version 13 in the way of hnrf_cloud.h: humannerf_amd/_lib.py binds these entries on first use
 * (load_heads) and raises when the library lacks them.
 *
 * The reference's CanonicalMLP with multihead.enable, head_depth 1 (canonical_mlps/mlp_rgb_sigma.py:114-115, :180-193):
 * output_linear.0 is (4 H, 256) and head g is its rows 4g .. 4g+3.  The reference gets H heads by H full passes
 * (test.head_id = g) or by its head_id = -1 list; here the trunk runs once.  The head layer of both inference kernels
 * is one 32-row MFMA tile either way, so 2 <= H <= 8 heads cost the single-head launch plus H - 1 more raw planes.
 * The usual convention: raw device pointers, sizes, a stream, int error codes, no allocation, no synchronisation; bad
 * arguments (H outside 2..8, a null plane, a misaligned raw) are refused before any launch.
 *
 * ---- hnrf_canonical_heads_pack: hnrf_canonical_pack for weights[8] (4 n_heads, 256), biases[8] (4 n_heads).
 *   Same image size (hnrf_canonical_packed_bytes) and same status word.  HNRF_MLP_F16X3: every head is lifted by a
 *   power of two of ITS OWN 4 x 256 weights, so that head g of hnrf_canonical_heads_fwd equals hnrf_canonical_fwd on
 *   the image hnrf_canonical_pack makes of rows 4g .. 4g+3, bit for bit.  An image of this entry is for the two
 *   entries below only (hnrf_canonical_fwd would read a bias where it expects the head's descale).
 *
 * ---- hnrf_canonical_heads_fwd / _sparse: hnrf_canonical_fwd / _sparse (mlp_rgb_sigma.py:180-193 with head_id = -1)
 *   with raw [n_heads][P][4], head-major planes: plane g is what hnrf_composite_fwd takes as the raw of head g.
 *   Sparse: the listed rows of every plane, nothing else; *count == 0 writes nothing.  mode as there (guard bits
 *   included: the status word and the guarded instances are the single-head ones).
 *
 * ---- hnrf_render_frame_heads_fwd: hnrf_render_frame_fwd (network.py:570-587: the per-head compositing of the
 *   head_id = -1 branch) with per-head outputs: K1 -> K2 -> K3 for all heads -> K4 once per head, per ray chunk.
 *   rgb, alpha, depth and the five per-head diagnostic outputs are HOST arrays of n_heads device pointers, each a
 *   whole-frame buffer of hnrf_render_frame_fwd's shape; weights_on_rays == NULL selects the lean form (then the other
 *   four arrays, xyz_on_rays and offsets are not read).  xyz_on_rays, bmw and offsets do not depend on the head: one
 *   buffer each.  workspace: hnrf_render_frame_heads_workspace_bytes(chunk, S, n_heads), 256-byte aligned.  Side
 *   stream, events and mlp_events as in hnrf_render_frame_fwd.  cull_eps > 0 in the lean form only, as there. */
#ifndef HNRF_HEADS_H
#define HNRF_HEADS_H

int hnrf_canonical_heads_pack(const float* const* weights, const float* const* biases, int n_heads, int mode,
                              void* packed, void* stream);
int hnrf_canonical_heads_fwd(const float* xyz, const void* packed, int mode, int64_t P, int n_heads, float* raw,
                             void* stream);
int hnrf_canonical_heads_fwd_sparse(const float* xyz, const void* packed, int mode, int64_t P, int n_heads,
                                    const int* idx, const int* count, float* raw, void* stream);
size_t hnrf_render_frame_heads_workspace_bytes(int64_t chunk, int S, int n_heads);
int hnrf_render_frame_heads_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                const float* vol, const float* bbox_min, const float* bbox_scale,
                                const float* hann_w, const void* nr_packed, const void* cnl_packed,
                                const float* bgcolor, int mode, float cull_eps, int64_t N, int S, int B, int G,
                                int64_t chunk, int n_heads, void* workspace, size_t workspace_bytes,
                                float* const* rgb, float* const* alpha, float* const* depth,
                                float* const* weights_on_rays, float* const* rgb_on_rays, float* const* cnl_xyz,
                                float* const* cnl_rgb, float* const* cnl_weight, float* xyz_on_rays, float* bmw,
                                float* offsets, void* side_stream, void* const* events, void* const* mlp_events,
                                void* stream);

#endif
