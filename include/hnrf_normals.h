/* libhnrf -- density-gradient normals: one observation-space normal per ray from the gradient of the density at the
 * ray's samples, the 8-bit normal / shaded panels painted from them, and the normal of the gated density a mesh is cut
 * from.  Included by hnrf.h (inside its extern "C"); additive to ABI version 13 in the way of hnrf_cloud.h:
 * humannerf_amd/_lib.py binds these entries on first use (load_normals) and raises when the library lacks them.
 *
 * The gradients themselves come from the training kernels (hnrf_canonical_fwd_train + hnrf_canonical_bwd with
 * d_raw = (0, 0, 0, 1), and hnrf_nonrigid_fwd_train + hnrf_nonrigid_bwd behind them): ops.density_gradient.  The entries
 * here are the HIP around them.  The usual convention: raw device pointers, sizes, a stream, int error codes, no
 * allocation, no synchronisation, no atomics on floats; bad arguments are refused before any launch and
 * hnrf_last_error names the argument.  All arithmetic is fp32, every operation rounded on its own (no fma; IEEE division
 * and square root), and humannerf_amd/geometry.py (ray_normals_host, normal_panels_host, field_normals_host) is the
 * numpy form of every statement below, bit for bit.
 *
 * ---- hnrf_ray_normals: the compositing-weighted mean of per-sample unit normals (Ref-NeRF), R rays of S samples.
 *   weights [R,S]; bmw [R,S,B] (backward_motion_weights); motion_Rs [B,3,3] row-major; idx [>= *count] int32, distinct,
 *   and count [1] int32 on the device: the kept samples as flat indices r S + s (hnrf_compact_samples(weights,
 *   weight_min): kept iff w >= weight_min; its order -- ascending within a block of samples, blocks as they arrive --
 *   does not matter here: row k of g belongs to sample idx[k], and a ray's sum runs over sample positions);
 *   g [*count,3] the density gradient in skeleton space at the kept samples, in idx order; alpha [R].  n_max = the
 *   capacity of idx and g (rows): *count > n_max is read as n_max; an index outside [0, R S) is skipped.
 *   Per kept sample:  A_ij = sum_b fl(bmw_b R_b[i][j]), b ascending from 0 (acc = fl(acc + fl(..)) from 0);
 *     v_j = -fl(fl(fl(A_0j g_0) + fl(A_1j g_1)) + fl(A_2j g_2))   (-A^T g: x_skel = A x_obs + t up to the positive
 *     weight sum, which only scales);  len = sqrt(fl(fl(fl(v_0 v_0) + fl(v_1 v_1)) + fl(v_2 v_2)));  a len that is 0
 *     or not finite contributes nothing;  otherwise u = v / len.
 *   Per ray:  N = sum_s w_s u_s over the kept samples in the order of hnrf_surface_points: lane l of 64 adds the samples
 *     l, l + 64, ... ascending (acc = fl(acc + fl(w u)) from 0), then the xor butterfly over the lane distances 32 .. 1.
 *     L = sqrt(fl(fl(fl(N_0 N_0) + fl(N_1 N_1)) + fl(N_2 N_2)));  normal = N / L, NOT flipped towards the camera (the
 *     sign of -grad sigma is information);  nvalid = (alpha finite and >= alpha_min) and L > 0 and finite;  normal = 0
 *     where the ray is not valid.
 *   One wave per ray, four per workgroup.  A wave finds its kept samples through a slot table [R,S] int32 in the
 *   workspace (-1 = not kept, else the row of g), cleared and written from idx by two launches in front.
 *   workspace: hnrf_ray_normals_workspace_bytes(R, S) bytes (0 for sizes refused), 256-byte aligned like every other
 *   workspace (a misaligned one is HNRF_E_ARG, a smaller one HNRF_E_WORKSPACE; either way nothing is written).  What it
 *   held before the call does not matter, and normal [R,3] / nvalid [R] are written whole: R floats x 3 and R bytes.
 *   idx and g are read on their first min(*count, n_max) rows only.
 *   R >= 0 (0 launches nothing), 1 <= S <= 512, 1 <= B <= 32, R S < 2^31, 0 <= n_max; alpha_min must not be NaN.
 *
 * ---- hnrf_normal_panels: the 8-bit panels from per-ray normals, one lane per pixel, lanes along x.
 *   pix2ray [H W] and status from hnrf_pixel_rays (a status word that is not 0: nothing is written); rays_d [N,3];
 *   ray_normal [N,3], ray_nvalid [N] from hnrf_ray_normals; valid [N] and surface as hnrf_geometry_maps takes them (a
 *   pixel is valid iff it has a ray whose bit `surface` of valid is set); alpha [N].  A pixel has a normal iff it is
 *   valid and its ray's ray_nvalid is not 0.  q8, (M n)_i, s, g and the blend are the statements of hnrf_geometry_maps:
 *     normal  [H,W,3] fp32 = the ray's normal, 0 where none;  nvalid [H,W] uint8
 *     normal8 [H,W,3] = q8(0.5 + 0.5 (M n)_i); q8(bgcolor) where there is no normal
 *     shaded8 [H,W,3] = q8(fl(fl(g a) + fl(fl(1 - a) bg_i))), g = fl(s albedo), s = ambient + (1 - ambient) |n.d| /
 *             sqrt(fl(fl(dx dx + dy dy) + dz dz)) with a normal (n.d = fl(fl(nx dx + ny dy) + nz dz)), ambient without;
 *             q8(bgcolor) on pixels that are not valid
 *   Each output nullable = not wanted; normal8 needs M [3,3]; shaded8 needs alpha.  1 <= H, W <= 16384, 0 <= N < 2^31.
 *
 * ---- hnrf_field_normals: the normal of D = relu(sigma) fg, fg the gate of hnrf_density_grid, one thread per vertex.
 *   verts [V,3] canonical; g [V,3] = grad sigma and sigma [V] at the vertices; vol [>= B,G,G,G]; bbox_min, bbox_scale [3].
 *   fg and the corner weights c_k = fl(fl(ux uy) uz) come from trilinear_at (csrc/hnrf_trilinear.h); fg = sum over b
 *   ascending of (w = 0; w = fl(w + fl(vol_b[corner k] c_k)), k = 0..7), as hnrf_density_grid.
 *   grad fg, the analytic derivative of those weights: per axis a, d_a c_k = fl(fl(e_x e_y) e_z) with e = the corner's
 *   weight on the other two axes and, on axis a, -1 for the lower node and +1 for the upper one where trilinear_at gives
 *   the node a weight (0 for a zero-padded node);  G_a = sum over b ascending of (w = 0; w = fl(w + fl(vol_b[corner k]
 *   d_a c_k)), k = 0..7);  (grad fg)_a = fl(G_a fl(fl(bbox_scale_a 0.5f) (G - 1))).
 *   grad D_a = fl(fl(fg gs_a) + fl(max(sigma, 0) (grad fg)_a)), gs = g where sigma > 0, else 0.
 *   len = sqrt(fl(fl(fl(D_0 D_0) + fl(D_1 D_1)) + fl(D_2 D_2)));  normal [V,3] = -grad D / len, 0 where len is 0 or not
 *   finite.  V >= 0 (0 launches nothing), 1 <= B <= 32, 2 <= G <= 1024. */
size_t hnrf_ray_normals_workspace_bytes(int64_t R, int S);
int hnrf_ray_normals(const float* weights, const float* bmw, const float* motion_Rs, const int* idx, const int* count,
                     int64_t n_max, const float* g, const float* alpha, int64_t R, int S, int B, float alpha_min,
                     void* workspace, size_t workspace_bytes, float* normal, uint8_t* nvalid, void* stream);
int hnrf_normal_panels(const float* rays_d, const float* ray_normal, const uint8_t* ray_nvalid, const uint8_t* valid,
                       int surface, const float* alpha, const int* pix2ray, int64_t N, int H, int W, const float* M,
                       const float* bgcolor, float ambient, float albedo, const int* status, float* normal,
                       uint8_t* nvalid, uint8_t* normal8, uint8_t* shaded8, void* stream);
int hnrf_field_normals(const float* verts, const float* g, const float* sigma, int64_t V, const float* vol, int B, int G,
                       const float* bbox_min, const float* bbox_scale, float* normal, void* stream);
