/* libhnrf -- view-dependent colour (canonical_mlp.view_dir, view_embed 'mlp'): the reference's view branch
 * (canonical_mlps/mlp_rgb_sigma.py:85-96, 168-178) has no non-linearity behind the trunk, so it folds into an ordinary
 * single-head canonical image plus three floats per RAY that are added to the raw colour in front of K4's sigmoid
 * (DESIGN.md section 4 "View-dependent colour").  Included by hnrf.h (inside its extern "C"); additive to ABI version 13
 * in the way of hnrf_cloud.h: humannerf_amd/_lib.py binds these entries on first use (load_view) and raises when the
 * library lacks them.  The usual convention: raw device pointers, sizes, a stream, int error codes, no allocation, no
 * synchronisation; bad arguments are refused before any launch and hnrf_last_error names the argument.  No entry here
 * uses atomics: the same inputs give the same bits.
 *
 * ---- hnrf_view_bias_fwd: bias [R,3] = B e(d) + c, one thread per ray.
 *   dirs [R,3] (any length); B [3, 3 + 6 L] row-major; c [3]; 1 <= L <= 10.
 *   n = d / max(|d|, 1e-12) (torch.nn.functional.normalize; |d| = sqrt(dx dx + dy dy + dz dz) in fp32, IEEE division and
 *   square root);  e(d) = (n, sin(2^0 n), cos(2^0 n), ..., sin(2^(L-1) n), cos(2^(L-1) n)), three values each -- the order
 *   of the reference's embedder (fourier.py);  bias_i = c_i + sum_j B_ij e_j, j ascending (acc from c_i).
 *   R >= 0 (0 launches nothing).
 *
 * ---- hnrf_view_bias_bwd: dB [3, 3 + 6 L] = sum_r d_bias[r] (x) e(d_r), dc [3] = sum_r d_bias[r].
 *   Two stages in a fixed order: stage one, a grid of (slices, 3 + 6 L + 1) workgroups of 256 threads, slices =
 *   min(64, ceil(R / 256)): thread t of slice s adds the rays s 256 + t, + slices 256, ... ascending for its column j
 *   (column 3 + 6 L is the constant 1 of dc), then the xor butterfly over the lane distances 32 .. 1 and the four waves
 *   ascending; stage two adds the slices ascending.  workspace: hnrf_view_bias_bwd_workspace_bytes(R, L) bytes (0 for
 *   sizes refused), 256-byte aligned.  dB and dc are written whole (zeros at R = 0).
 *
 * ---- hnrf_composite_view_fwd: hnrf_composite_fwd with view_bias [R,3] added to raw.xyz of every sample of the ray, one
 *   fp32 add in front of the sigmoid (rgb_on_rays and cnl_rgb carry it too).  view_bias null = hnrf_composite_fwd: the
 *   two are one kernel body, and hnrf_composite_fwd is this entry with a null bias.
 *
 * ---- hnrf_composite_view_bwd: hnrf_composite_bwd with the bias in its sigmoids; d_bias [R,3] (nullable) receives
 *   sum_s d_raw[r, s].xyz: every lane adds its own samples descending, then the xor butterfly over 32 .. 1.
 *   view_bias null = hnrf_composite_bwd (d_bias may still be asked for).
 *
 * ---- hnrf_render_frame_view_fwd: the ONE frame entry of the view path.  The arguments of hnrf_render_frame_fwd, and
 *   -- each nullable, null = as in hnrf_render_frame_fwd --
 *     off_grid, off_M, off_bbox_min, off_bbox_max   the offset grid of hnrf_render_frame_baked_nr_fwd (then hann_w and
 *                                                   nr_packed are not read; needs grid)
 *     grid, grid_N, grid_bbox_min, grid_bbox_max    the canonical grid of hnrf_render_frame_baked_fwd (then cnl_packed is
 *                                                   not read)
 *     view_bias [N,3]                               added in every chunk's K4
 *     live_counts [ceil(N / chunk)]                 the shared evaluation of hnrf_render_frame_shared_fwd, with its
 *                                                   workspace size and its conditions
 *   With view_bias null (or all zero up to the sign of a zero raw colour, which the sigmoid does not see) every output
 *   equals that of the entry the other arguments select, bit for bit. */
int hnrf_view_bias_fwd(const float* dirs, const float* B, const float* c, int L, int64_t R, float* bias, void* stream);
size_t hnrf_view_bias_bwd_workspace_bytes(int64_t R, int L);
int hnrf_view_bias_bwd(const float* dirs, const float* d_bias, int L, int64_t R, void* workspace, size_t workspace_bytes,
                       float* dB, float* dc, void* stream);
int hnrf_composite_view_fwd(const float* raw, const float* fg_mask, const float* z_vals, const float* rays_d,
                            const float* xyz, const float* bgcolor, const float* view_bias, int64_t R, int S,
                            float cull_eps, float* rgb, float* alpha, float* depth, float* weights, float* rgb_on_rays,
                            float* cnl_xyz, float* cnl_rgb, float* cnl_weight, void* stream);
int hnrf_composite_view_bwd(const float* raw, const float* fg_mask, const float* z_vals, const float* rays_d,
                            const float* bgcolor, const float* view_bias, const float* g_rgb, const float* g_alpha,
                            const float* g_depth, int64_t R, int S, float* d_raw, float* d_mask, float* d_bias,
                            void* stream);
int hnrf_render_frame_view_fwd(const float* rays_o, const float* rays_d, const float* near, const float* far,
                               const float* t_rand, const float* motion_Rs, const float* motion_Ts, const float* vol,
                               const float* bbox_min, const float* bbox_scale, const float* hann_w, const void* nr_packed,
                               const void* cnl_packed, const void* off_grid, int off_M, const float* off_bbox_min,
                               const float* off_bbox_max, const void* grid, int grid_N, const float* grid_bbox_min,
                               const float* grid_bbox_max, const float* view_bias, const float* bgcolor, int mode,
                               float cull_eps, int64_t N, int S, int B, int G, int64_t chunk, void* workspace,
                               size_t workspace_bytes, float* rgb, float* alpha, float* depth, float* weights_on_rays,
                               float* rgb_on_rays, float* cnl_xyz, float* cnl_rgb, float* cnl_weight, float* xyz_on_rays,
                               float* bmw, float* offsets, int* live_counts, void* side_stream, void* const* events,
                               void* const* mlp_events, void* stream);
