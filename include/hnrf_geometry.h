/* libhnrf -- geometry maps of a rendered frame: depth, normal, shaded and non-rigid-offset panels.  Included by hnrf.h
 * (inside its extern "C"); additive to ABI version 13 in the way of hnrf_cloud.h: humannerf_amd/_lib.py binds these
 * entries on first use (load_geometry) and raises when the library lacks them.
 *
 * The normals are SCREEN-SPACE DIFFERENCES OF THE RENDERED SURFACE DISTANCE: no network evaluation, no density gradient.
 * The usual convention: raw device pointers, sizes, a stream, int error codes, no allocation, no synchronisation; bad
 * arguments are refused before any launch and hnrf_last_error names the argument.  All arithmetic is fp32, every
 * operation rounded on its own (no fma; IEEE division and square root), and humannerf_amd/geometry.py (ray_surface_host,
 * pixel_rays_host, maps_host) is the numpy form of every statement below, bit for bit.  Defined for unperturbed
 * sampling (cfg.perturb == 0): only then do the samples sit at z_at.
 *
 * ---- hnrf_ray_surface: the surface distance of R rays of S samples, 1 <= S <= 65536, 0 <= R, R S < 2^40.
 *   alpha, depth [R] from the compositing kernel; near, far [R]; weights [R,S] and offsets [R,S,3] nullable (lean form).
 *   valid [R] uint8: bit 0 = t_exp is a surface, bit 1 = t_med is.  A distance that is no surface is written as 0.
 *   t_exp = depth / alpha where alpha and depth are finite and alpha >= alpha_min.
 *   t_med = z_k, k the first sample whose inclusive cumulative weight c_k >= 0.5f * c_{S-1}; z_k = K1's statement of a
 *     sample's depth (csrc/hnrf_zat.h).  It needs bit 0, c_{S-1} > 0, a k that qualifies (a NaN among the weights makes
 *     every comparison false) and a finite z_k (S = 1 has none: the lerp parameter is 0 / 0).
 *     The cumulative sum, an order that depends on S alone: tiles of 64 samples ascending; within a tile the Kogge-Stone
 *     inclusive scan v_k += v_{k-off} for off = 1, 2, 4, 8, 16, 32 where k >= off (samples past S count as 0); then
 *     c_k = fl(carry + v_k), and carry = c of the tile's last lane (0 before the first tile).
 *   woff [R,3] = sum_s w_s offset_s: lane l of 64 adds the samples l, l + 64, ... ascending (acc = fl(acc + fl(w x))),
 *     then the xor butterfly over the lane distances 32, 16 .. 1 -- the order of hnrf_surface_points.
 *   One wave per ray, four per workgroup (lean form: one lane per ray).  t_exp, t_med, woff are nullable = not wanted;
 *   t_med or woff without weights (woff: without offsets) is refused.  alpha_min must not be NaN.
 *
 * ---- hnrf_pixel_rays: pix2ray [H W] int32 = the ray of every pixel, -1 where there is none.
 *   ray_index [N] int64 = the flat pixel of ray n; 1 <= H, W <= 16384, 0 <= N < 2^31.  Two rays on one pixel: the
 *   highest n (an integer atomic max: the result does not depend on the order of execution).
 *   status [1] int32 (the convention of hnrf_segment.h): zeroed, then written by the first launch, 0 = fine,
 *     1  an index outside [0, H W).
 *   The later launches of this entry and those of hnrf_geometry_maps given the same word read it on the device and
 *   write NOTHING when it is not 0 (pix2ray keeps whatever it held).
 *
 * ---- hnrf_geometry_maps: the panels, one lane per pixel, lanes along x.
 *   rays_o, rays_d [N,3] as given to the network (not normalised); t_exp / t_med / valid / woff from hnrf_ray_surface;
 *   surface 0 = t_exp and bit 0 of valid, 1 = t_med and bit 1.  A pixel is valid iff it has a ray whose bit is set.
 *   P = o + d t per component, fl(o + fl(d t)).
 *   Per image axis (x = column, y = row) with the neighbours m (minus) and p (plus); a neighbour QUALIFIES iff it lies
 *   in the image, is valid and |t_n - t| <= edge:  D = P_p - P_m if both qualify, else P_p - P if p does, else
 *   P - P_m if m does, else the pixel has no normal.
 *   c = cross(D_x, D_y), each component fl(fl(a b) - fl(c d)); len = sqrt(fl(fl(cx cx + cy cy) + cz cz)); a len that is
 *   0 or not finite gives no normal; n = c / len, negated when n.d = fl(fl(nx dx + ny dy) + nz dz) > 0 (it faces the
 *   camera).  edge >= 0.
 *   q8(v) = 0 where !(v > 0), 255 where v >= 1, else trunc(255 v): render.to_8b_image, with NaN -> 0.
 *   Outputs, each nullable = not wanted; bgcolor [3] in 0..1:
 *     normal  [H,W,3] fp32 world space, 0 where none;  nvalid [H,W] uint8
 *     normal8 [H,W,3] = q8(0.5 + 0.5 (M n)_i), (M n)_i = fl(fl(M_i0 nx + M_i1 ny) + M_i2 nz), M [3,3] row-major (the
 *             world-to-camera rotation: the rasteriser's shade = 'normal'); q8(bgcolor) where there is no normal
 *     depth8  [H,W,3] = gray q8(1 - (t - lo) / (hi - lo)) on valid pixels, lohi [2] = {lo, hi} read on the device;
 *             q8(bgcolor) elsewhere
 *     shaded8 [H,W,3] = q8(fl(fl(g a) + fl(fl(1 - a) bg_i))), a = the ray's alpha, g = fl(s albedo),
 *             s = ambient + (1 - ambient) |n.d| / sqrt(fl(fl(dx dx + dy dy) + dz dz)) with a normal, ambient without;
 *             q8(bgcolor) on pixels that are not valid
 *     offset8 [H,W,3] = trunc(255 clip((woff_i - (-0.02f)) / 0.04f, 0, 1)) (NaN -> 0): compare_lbs_delta.py:7-9, 41-47
 *             of the reference; painted where the pixel has a ray and (truth8 [H,W,3] given: its three channels sum
 *             to > 0; truth8 null: the pixel is valid), 0 elsewhere.
 *   status nullable. */
int hnrf_ray_surface(const float* near, const float* far, const float* alpha, const float* depth, const float* weights,
                     const float* offsets, int64_t R, int S, float alpha_min, float* t_exp, float* t_med, float* woff,
                     uint8_t* valid, void* stream);
int hnrf_pixel_rays(const int64_t* ray_index, int64_t N, int H, int W, int* pix2ray, int* status, void* stream);
int hnrf_geometry_maps(const float* rays_o, const float* rays_d, const float* t_exp, const float* t_med,
                       const uint8_t* valid, int surface, const float* alpha, const float* woff, const int* pix2ray,
                       int64_t N, int H, int W, float edge, const float* M, const float* bgcolor, const float* lohi,
                       float ambient, float albedo, const uint8_t* truth8, const int* status, float* normal,
                       uint8_t* nvalid, uint8_t* normal8, uint8_t* depth8, uint8_t* shaded8, uint8_t* offset8,
                       void* stream);
