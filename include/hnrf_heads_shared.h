/* libhnrf -- every head of a multi-head canonical image with the shared evaluation of underflowing inputs: the samples
 * whose MLP inputs are those of x_skel = 0 (the predicate: hnrf.h at hnrf_share_compact) are evaluated once per frame
 * for ALL heads.  Included by hnrf.h (inside its extern "C"); additive to ABI version 13 in the way of hnrf_heads.h:
 * humannerf_amd/_lib.py binds these entries on first use (load_heads_shared, table OPEN_GROUPS) and raises when the
 * library lacks them.
 *
 * Nothing in the predicate depends on the head: a sample is shared because of x_skel, c_off and c_xyz, which K1 and K2
 * decide.  What depends on the head is the representative's canonical output: c_raw is [n_heads][4], head g's four
 * values at c_raw + 4 g -- what hnrf_canonical_heads_fwd writes for P = 1 -- and a shared sample p gets c_raw[g] in
 * plane g of raw [n_heads][P][4], the head-major planes hnrf_canonical_heads_fwd_sparse then fills on the live list.
 * offsets and xyz are one buffer each, as in hnrf_heads.h.  The usual convention: raw device pointers, sizes, a stream,
 * int error codes, no allocation, no synchronisation; 2 <= n_heads <= 8; bad arguments are refused before any launch.
 *
 * ---- hnrf_share_compact_heads: hnrf_share_compact with n_heads, c_raw [n_heads][4] and raw [n_heads][P][4].
 *   idx[0 .. *count) = the live samples, each listed ONCE (count zeroed and written on the device); for every shared p
 *   and every head g: raw[g][p] = c_raw[g], one 16-byte store per plane; offsets[p] = c_off, xyz[p] = c_xyz once (both
 *   NULL = not written).  No plane row of a live sample is touched.  HNRF_E_ARG: n_heads outside 2..8, a null pointer,
 *   offsets without xyz, P < 0 or >= 2^31 - 1, raw not 16-byte aligned.  P == 0 sets *count = 0 without a launch.
 *
 * ---- hnrf_sample_warp_share_heads_fwd: hnrf_sample_warp_share_fwd (K1 with the classification fused in) with the same
 *   three arguments changed; P = R S, the planes R S rows apart.  z_vals / x_skel / fg_mask / bmw, idx and count are
 *   what hnrf_sample_warp_share_fwd writes, bit for bit.  HNRF_E_UNSUPPORTED for any bone count but 24, then the
 *   refusals above.
 *
 * ---- hnrf_render_frame_heads_shared_workspace_bytes(chunk, S, n_heads): the workspace of the entry below -- the two
 *   chunk workspaces, the 256 bytes of the representative slot (x | c_off | c_xyz | c_raw [n_heads][4] from float 12),
 *   and TWO sets of n_heads raw planes of one chunk.  Two, where hnrf_render_frame_heads_fwd has one: with a side stream
 *   K1 of chunk i+1 writes the shared rows of its planes while the compositing passes of chunk i still read theirs, so
 *   the sets alternate like the chunk workspaces.  0 for n_heads outside 2..8 or a negative size.
 *
 * ---- hnrf_render_frame_heads_shared_fwd: hnrf_render_frame_heads_fwd with every chunk as hnrf_render_frame_shared_fwd
 *   runs it: K1 with the classification fused in (any bone count but 24: K1 -> the compaction above on `stream`) -> K2
 *   and K3 for all heads on the live list -> K4 once per head; the representative through K2 and the all-heads K3 once
 *   per frame in front of chunk 0, by the chunks' kernel instances (guarded unless HNRF_MLP_NO_RANGE_GUARD; no
 *   mlp_events around it).  Every output equals hnrf_render_frame_heads_fwd's bit for bit.  Arguments as there, plus
 *   live_counts [ceil(N / chunk)] (device, required): the number of samples of each chunk that went through the MLPs
 *   (once, not once per head).  Refused: live_counts NULL, n_heads outside 2..8, a null plane or output array
 *   (HNRF_E_ARG); a workspace under the stated size (HNRF_E_WORKSPACE); a mode that is not HNRF_MLP_F16X3, nr_packed
 *   NULL, cull_eps != 0 (HNRF_E_UNSUPPORTED).  The caller checks that every Hann weight is <= 1, as for
 *   hnrf_render_frame_shared_fwd. */
#ifndef HNRF_HEADS_SHARED_H
#define HNRF_HEADS_SHARED_H

int hnrf_share_compact_heads(const float* x_skel, const float* c_off, const float* c_xyz, const float* c_raw, int64_t P,
                             int n_heads, int* idx, int* count, float* offsets, float* xyz, float* raw, void* stream);
int hnrf_sample_warp_share_heads_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                     const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                     const float* vol, const float* bbox_min, const float* bbox_scale, int64_t R, int S,
                                     int B, int G, float* z_vals, float* x_skel, float* fg_mask, float* bmw,
                                     const float* c_off, const float* c_xyz, const float* c_raw, int n_heads, int* idx,
                                     int* count, float* offsets, float* xyz, float* raw, void* stream);
size_t hnrf_render_frame_heads_shared_workspace_bytes(int64_t chunk, int S, int n_heads);
int hnrf_render_frame_heads_shared_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                                       const float* t_rand, const float* motion_Rs, const float* motion_Ts,
                                       const float* vol, const float* bbox_min, const float* bbox_scale,
                                       const float* hann_w, const void* nr_packed, const void* cnl_packed,
                                       const float* bgcolor, int mode, float cull_eps, int64_t N, int S, int B, int G,
                                       int64_t chunk, int n_heads, void* workspace, size_t workspace_bytes,
                                       float* const* rgb, float* const* alpha, float* const* depth,
                                       float* const* weights_on_rays, float* const* rgb_on_rays, float* const* cnl_xyz,
                                       float* const* cnl_rgb, float* const* cnl_weight, float* xyz_on_rays, float* bmw,
                                       float* offsets, int* live_counts, void* side_stream, void* const* events,
                                       void* const* mlp_events, void* stream);

#endif
