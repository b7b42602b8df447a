// Geometry maps of a rendered frame (hnrf_geometry.h; humannerf_amd/geometry.py is the numpy twin of every statement
// here, bit for bit): the surface distance per ray, the pixel -> ray map, and the depth / normal / shaded / offset
// panels.  The normals are screen-space differences of the rendered surface distance.
//
//   ray_surface_kernel   one wave per ray (4 per workgroup, as surface_points_kernel and K4).  The weights are read
//                        three times as coalesced 256-byte rows (the second and third time from L2): once lane-strided
//                        with the offsets for woff, once for the total of the tiled Kogge-Stone scan, once more to find
//                        the first sample at or above half of it (a ballot per tile).
//   ray_expected_kernel  the lean form: no per-sample input, one lane per ray.
//   pixel_check_kernel   one lane per ray: an index outside the image raises the status word, which every later kernel
//                        reads first and, when it is not 0, returns without writing.
//   pixel_clear_kernel   pix2ray = -1;  pixel_set_kernel: atomicMax(pix2ray + ray_index[n], n).
//   geometry_maps_kernel one lane per pixel, 64 x 4 pixels per workgroup, lanes along x: the pixel's and its four
//                        neighbours' rays are gathered through pix2ray (rays come in pixel order, so a wave's gathers
//                        fall on neighbouring 28 bytes; the 7 MB of a 512 x 512 frame stay in L2).
// Compiled without contraction and with the correctly rounded division and square root (Makefile).  No LDS.
#include "hnrf_common.h"
#include "hnrf_zat.h"

namespace hnrf {

constexpr int kGeoMaxSide = 16384, kGeoMaxS = 65536;
constexpr int64_t kGeoMaxRays = ((int64_t)1 << 31) - 1;
constexpr int64_t kGeoMaxSamples = (int64_t)1 << 40;
enum { kGeoOutside = 1 };

__device__ __forceinline__ bool geo_finite(float v) { return fabsf(v) < __builtin_inff(); }        // (NaN: false)

// t_exp and bit 0 of valid
__device__ __forceinline__ float geo_expected(float a, float d, float alpha_min, bool* ok) {
    *ok = geo_finite(a) && geo_finite(d) && a >= alpha_min;
    return *ok ? d / a : 0.f;
}

__global__ __launch_bounds__(256) void ray_expected_kernel(const float* __restrict__ alpha, const float* __restrict__ depth,
                                                           int64_t R, float alpha_min, float* __restrict__ t_exp,
                                                           uint8_t* __restrict__ valid) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    bool ok;
    const float t = geo_expected(alpha[r], depth[r], alpha_min, &ok);
    if (t_exp) t_exp[r] = t;
    valid[r] = ok ? 1 : 0;
}

// one tile of the cumulative sum: v = this lane's weight (0 past S) -> c of this lane; carry moves on to the tile's end
__device__ __forceinline__ float geo_scan_tile(float v, int lane, float* carry) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float u = __shfl_up(v, off, 64);
        if (lane >= off) v = v + u;
    }
    const float c = *carry + v;
    *carry = __shfl(c, 63, 64);
    return c;
}

__global__ __launch_bounds__(256) void ray_surface_kernel(const float* __restrict__ near, const float* __restrict__ far,
                                                          const float* __restrict__ alpha, const float* __restrict__ depth,
                                                          const float* __restrict__ weights, const float* __restrict__ offsets,
                                                          int64_t R, int S, float alpha_min, float* __restrict__ t_exp,
                                                          float* __restrict__ t_med, float* __restrict__ woff,
                                                          uint8_t* __restrict__ valid) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= R) return;   // wave-uniform
    const int64_t base = ray * S;
    bool ok;
    const float te = geo_expected(alpha[ray], depth[ray], alpha_min, &ok);
    if (woff) {
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int s = lane; s < S; s += 64) {
            const float w = weights[base + s];
            const float* p = offsets + (base + s) * 3;
            sx = sx + w * p[0];
            sy = sy + w * p[1];
            sz = sz + w * p[2];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            sx = sx + __shfl_xor(sx, off, 64);
            sy = sy + __shfl_xor(sy, off, 64);
            sz = sz + __shfl_xor(sz, off, 64);
        }
        if (lane == 0) {
            woff[ray * 3 + 0] = sx;
            woff[ray * 3 + 1] = sy;
            woff[ray * 3 + 2] = sz;
        }
    }
    float tm = 0.f;
    bool okm = false;
    if (t_med && ok) {      // wave-uniform
        float carry = 0.f, c_last = 0.f;
        for (int s0 = 0; s0 < S; s0 += 64)
            c_last = geo_scan_tile(s0 + lane < S ? weights[base + s0 + lane] : 0.f, lane, &carry);
        // c_{S-1}, from its own lane: the last lane of a ragged tile adds the same terms in another grouping
        const float total = __shfl(c_last, (S - 1) & 63, 64);
        if (total > 0.f) {
            const float thr = 0.5f * total;
            carry = 0.f;
            int k = -1;
            for (int s0 = 0; s0 < S && k < 0; s0 += 64) {
                const bool in = s0 + lane < S;
                const float c = geo_scan_tile(in ? weights[base + s0 + lane] : 0.f, lane, &carry);
                const unsigned long long hit = __ballot(in && c >= thr);
                if (hit) k = s0 + (int)__ffsll((long long)hit) - 1;
            }
            if (k >= 0) {
                const float z = z_at(near[ray], far[ray], k, S);
                if (geo_finite(z)) { tm = z; okm = true; }
            }
        }
    }
    if (lane == 0) {
        if (t_exp) t_exp[ray] = te;
        if (t_med) t_med[ray] = tm;
        valid[ray] = (ok ? 1 : 0) | (okm ? 2 : 0);
    }
}

// ---- pixel -> ray
__global__ __launch_bounds__(256) void pixel_check_kernel(const int64_t* __restrict__ ray_index, int64_t N, int64_t HW,
                                                          int* __restrict__ status) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = n < N && (ray_index[n] < 0 || ray_index[n] >= HW);
    if (__ballot(bad) == 0) return;                                      // wave-uniform: the usual case
    if (bad) atomicOr(status, (int)kGeoOutside);
}

__global__ __launch_bounds__(256) void pixel_clear_kernel(int* __restrict__ pix2ray, int64_t HW, const int* __restrict__ status) {
    if (*status != 0) return;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < HW) pix2ray[p] = -1;
}

__global__ __launch_bounds__(256) void pixel_set_kernel(const int64_t* __restrict__ ray_index, int64_t N, int64_t HW,
                                                        int* __restrict__ pix2ray, const int* __restrict__ status) {
    if (*status != 0) return;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int64_t p = ray_index[n];
    if (p >= 0 && p < HW) atomicMax(pix2ray + p, (int)n);
}

// ---- maps
struct GeoPix {
    bool ok;              // the pixel has a ray whose surface bit is set
    int ray;              // its ray, -1 = none
    float t, px, py, pz;
};

__device__ __forceinline__ GeoPix geo_pixel(int x, int y, int H, int W, int64_t N, const int* __restrict__ pix2ray,
                                            const float* __restrict__ o, const float* __restrict__ d,
                                            const float* __restrict__ t, const uint8_t* __restrict__ valid, int bit) {
    GeoPix g{false, -1, 0.f, 0.f, 0.f, 0.f};
    if (x < 0 || x >= W || y < 0 || y >= H) return g;
    const int r = pix2ray[(int64_t)y * W + x];
    if (r < 0 || r >= N) return g;
    g.ray = r;
    if (!((valid[r] >> bit) & 1)) return g;
    g.ok = true;
    g.t = t[r];
    g.px = o[(int64_t)r * 3 + 0] + d[(int64_t)r * 3 + 0] * g.t;
    g.py = o[(int64_t)r * 3 + 1] + d[(int64_t)r * 3 + 1] * g.t;
    g.pz = o[(int64_t)r * 3 + 2] + d[(int64_t)r * 3 + 2] * g.t;
    return g;
}

// the difference along one image axis; false = none
__device__ __forceinline__ bool geo_diff(const GeoPix& c, const GeoPix& m, const GeoPix& p, float edge, float* dx, float* dy,
                                         float* dz) {
    const bool qm = m.ok && fabsf(c.t - m.t) <= edge, qp = p.ok && fabsf(p.t - c.t) <= edge;
    if (!qm && !qp) return false;
    const GeoPix& a = qp ? p : c;
    const GeoPix& b = qm ? m : c;
    *dx = a.px - b.px;
    *dy = a.py - b.py;
    *dz = a.pz - b.pz;
    return true;
}

__device__ __forceinline__ uint8_t geo_q8(float v) {
    return !(v > 0.f) ? (uint8_t)0 : v >= 1.f ? (uint8_t)255 : (uint8_t)(int)(255.f * v);
}

__device__ __forceinline__ void geo_put3(uint8_t* __restrict__ img, int64_t pix, uint8_t a, uint8_t b, uint8_t c) {
    img[pix * 3 + 0] = a;
    img[pix * 3 + 1] = b;
    img[pix * 3 + 2] = c;
}

__global__ __launch_bounds__(256) void geometry_maps_kernel(
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ t,
    const uint8_t* __restrict__ valid, int bit, const float* __restrict__ alpha, const float* __restrict__ woff,
    const int* __restrict__ pix2ray, int64_t N, int H, int W, float edge, const float* __restrict__ M,
    const float* __restrict__ bgcolor, const float* __restrict__ lohi, float ambient, float albedo,
    const uint8_t* __restrict__ truth8, const int* __restrict__ status, float* __restrict__ normal,
    uint8_t* __restrict__ nvalid, uint8_t* __restrict__ normal8, uint8_t* __restrict__ depth8, uint8_t* __restrict__ shaded8,
    uint8_t* __restrict__ offset8) {
    if (status && *status != 0) return;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int64_t pix = (int64_t)y * W + x;
    const GeoPix c = geo_pixel(x, y, H, W, N, pix2ray, rays_o, rays_d, t, valid, bit);
    const uint8_t bg0 = geo_q8(bgcolor[0]), bg1 = geo_q8(bgcolor[1]), bg2 = geo_q8(bgcolor[2]);

    bool has = false;
    float nx = 0.f, ny = 0.f, nz = 0.f, nd = 0.f, dl = 0.f;
    const bool want_n = normal || nvalid || normal8 || shaded8;
    if (c.ok && want_n) {
        const GeoPix xm = geo_pixel(x - 1, y, H, W, N, pix2ray, rays_o, rays_d, t, valid, bit);
        const GeoPix xp = geo_pixel(x + 1, y, H, W, N, pix2ray, rays_o, rays_d, t, valid, bit);
        const GeoPix ym = geo_pixel(x, y - 1, H, W, N, pix2ray, rays_o, rays_d, t, valid, bit);
        const GeoPix yp = geo_pixel(x, y + 1, H, W, N, pix2ray, rays_o, rays_d, t, valid, bit);
        float ax, ay, az, bx, by, bz;
        if (geo_diff(c, xm, xp, edge, &ax, &ay, &az) && geo_diff(c, ym, yp, edge, &bx, &by, &bz)) {
            const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
            if (len > 0.f && geo_finite(len)) {
                has = true;
                nx = cx / len;
                ny = cy / len;
                nz = cz / len;
                const float d0 = rays_d[(int64_t)c.ray * 3 + 0], d1 = rays_d[(int64_t)c.ray * 3 + 1],
                            d2 = rays_d[(int64_t)c.ray * 3 + 2];
                nd = (nx * d0 + ny * d1) + nz * d2;
                if (nd > 0.f) { nx = -nx; ny = -ny; nz = -nz; }
                dl = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
            }
        }
    }
    if (normal) {
        normal[pix * 3 + 0] = nx;
        normal[pix * 3 + 1] = ny;
        normal[pix * 3 + 2] = nz;
    }
    if (nvalid) nvalid[pix] = has ? 1 : 0;
    if (normal8) {
        if (has) {
            uint8_t q[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) q[i] = geo_q8(0.5f + 0.5f * ((M[i * 3] * nx + M[i * 3 + 1] * ny) + M[i * 3 + 2] * nz));
            geo_put3(normal8, pix, q[0], q[1], q[2]);
        } else {
            geo_put3(normal8, pix, bg0, bg1, bg2);
        }
    }
    if (depth8) {
        if (c.ok) {
            const float lo = lohi[0], hi = lohi[1];
            const uint8_t g = geo_q8(1.f - (c.t - lo) / (hi - lo));
            geo_put3(depth8, pix, g, g, g);
        } else {
            geo_put3(depth8, pix, bg0, bg1, bg2);
        }
    }
    if (shaded8) {
        if (c.ok) {
            const float s = has ? ambient + (1.f - ambient) * (fabsf(nd) / dl) : ambient;
            const float g = s * albedo, a = alpha[c.ray], ga = g * a, na = 1.f - a;
            geo_put3(shaded8, pix, geo_q8(ga + na * bgcolor[0]), geo_q8(ga + na * bgcolor[1]), geo_q8(ga + na * bgcolor[2]));
        } else {
            geo_put3(shaded8, pix, bg0, bg1, bg2);
        }
    }
    if (offset8) {
        bool paint = c.ray >= 0;
        if (paint && truth8) paint = (int)truth8[pix * 3] + (int)truth8[pix * 3 + 1] + (int)truth8[pix * 3 + 2] > 0;
        else if (paint) paint = c.ok;
        uint8_t q[3] = {0, 0, 0};
        if (paint) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float v = (woff[(int64_t)c.ray * 3 + i] - (-0.02f)) / 0.04f;
                const float vc = !(v > 0.f) ? 0.f : v > 1.f ? 1.f : v;
                q[i] = (uint8_t)(int)(vc * 255.f);
            }
        }
        geo_put3(offset8, pix, q[0], q[1], q[2]);
    }
}

}  // namespace hnrf

using namespace hnrf;

extern "C" int hnrf_ray_surface(const float* near, const float* far, const float* alpha, const float* depth,
                                const float* weights, const float* offsets, int64_t R, int S, float alpha_min, float* t_exp,
                                float* t_med, float* woff, uint8_t* valid, void* stream) {
    HNRF_REQUIRE(S >= 1 && S <= kGeoMaxS, HNRF_E_ARG, "hnrf_ray_surface: S %d (1 .. %d)", S, kGeoMaxS);
    HNRF_REQUIRE(R >= 0 && R <= kGeoMaxRays && R * (int64_t)S < kGeoMaxSamples, HNRF_E_ARG,
                 "hnrf_ray_surface: R %lld of S %d samples", (long long)R, S);
    HNRF_REQUIRE(alpha_min == alpha_min, HNRF_E_ARG, "hnrf_ray_surface: alpha_min is NaN");
    HNRF_REQUIRE(!t_med || weights, HNRF_E_ARG, "hnrf_ray_surface: t_med needs weights (the lean form has t_exp only)");
    HNRF_REQUIRE(!woff || (weights && offsets), HNRF_E_ARG,
                 "hnrf_ray_surface: woff needs weights and offsets (the lean form has t_exp only)");
    HNRF_REQUIRE(!t_med || (near && far), HNRF_E_ARG, "hnrf_ray_surface: t_med needs near and far");
    if (R == 0) return HNRF_OK;
    HNRF_REQUIRE(alpha && depth && valid, HNRF_E_ARG, "hnrf_ray_surface: null pointer (alpha, depth, valid)");
    hipStream_t st = (hipStream_t)stream;
    if (!t_med && !woff)
        hipLaunchKernelGGL(ray_expected_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, alpha, depth, R, alpha_min,
                           t_exp, valid);
    else
        hipLaunchKernelGGL(ray_surface_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, near, far, alpha, depth, weights,
                           offsets, R, S, alpha_min, t_exp, t_med, woff, valid);
    return check_launch("hnrf_ray_surface");
}

static int geo_image_ok(const char* who, int64_t N, int H, int W) {
    HNRF_REQUIRE(H >= 1 && H <= kGeoMaxSide, HNRF_E_ARG, "%s: H %d (1 .. %d)", who, H, kGeoMaxSide);
    HNRF_REQUIRE(W >= 1 && W <= kGeoMaxSide, HNRF_E_ARG, "%s: W %d (1 .. %d)", who, W, kGeoMaxSide);
    HNRF_REQUIRE(N >= 0 && N <= kGeoMaxRays, HNRF_E_ARG, "%s: N %lld (0 .. 2^31 - 1)", who, (long long)N);
    return HNRF_OK;
}

extern "C" int hnrf_pixel_rays(const int64_t* ray_index, int64_t N, int H, int W, int* pix2ray, int* status, void* stream) {
    if (int rc = geo_image_ok("hnrf_pixel_rays", N, H, W)) return rc;
    HNRF_REQUIRE(pix2ray && status && (N == 0 || ray_index), HNRF_E_ARG, "hnrf_pixel_rays: null pointer");
    HNRF_REQUIRE(((uintptr_t)ray_index & 7) == 0 && ((uintptr_t)pix2ray & 3) == 0 && ((uintptr_t)status & 3) == 0, HNRF_E_ARG,
                 "hnrf_pixel_rays: ray_index must be 8-byte aligned, pix2ray and status 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
        set_error("hnrf_pixel_rays: hipMemsetAsync failed");
        return HNRF_E_LAUNCH;
    }
    const int64_t HW = (int64_t)H * W;
    if (N > 0)
        hipLaunchKernelGGL(pixel_check_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, ray_index, N, HW, status);
    hipLaunchKernelGGL(pixel_clear_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, st, pix2ray, HW, (const int*)status);
    if (N > 0)
        hipLaunchKernelGGL(pixel_set_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, ray_index, N, HW, pix2ray,
                           (const int*)status);
    return check_launch("hnrf_pixel_rays");
}

extern "C" int hnrf_geometry_maps(const float* rays_o, const float* rays_d, const float* t_exp, const float* t_med,
                                  const uint8_t* valid, int surface, const float* alpha, const float* woff,
                                  const int* pix2ray, int64_t N, int H, int W, float edge, const float* M,
                                  const float* bgcolor, const float* lohi, float ambient, float albedo, const uint8_t* truth8,
                                  const int* status, float* normal, uint8_t* nvalid, uint8_t* normal8, uint8_t* depth8,
                                  uint8_t* shaded8, uint8_t* offset8, void* stream) {
    if (int rc = geo_image_ok("hnrf_geometry_maps", N, H, W)) return rc;
    HNRF_REQUIRE(surface == 0 || surface == 1, HNRF_E_ARG, "hnrf_geometry_maps: surface %d (0 = expected, 1 = median)", surface);
    HNRF_REQUIRE(edge >= 0.f, HNRF_E_ARG, "hnrf_geometry_maps: edge must be >= 0 (and no NaN)");
    HNRF_REQUIRE(ambient == ambient && albedo == albedo, HNRF_E_ARG, "hnrf_geometry_maps: ambient or albedo is NaN");
    const float* t = surface ? t_med : t_exp;
    HNRF_REQUIRE(pix2ray && bgcolor, HNRF_E_ARG, "hnrf_geometry_maps: null pointer (pix2ray, bgcolor)");
    HNRF_REQUIRE(N == 0 || (rays_o && rays_d && valid), HNRF_E_ARG, "hnrf_geometry_maps: null pointer (rays_o, rays_d, valid)");
    HNRF_REQUIRE(N == 0 || t, HNRF_E_ARG, "hnrf_geometry_maps: null pointer (%s, the surface asked for)", surface ? "t_med" : "t_exp");
    HNRF_REQUIRE(!normal8 || M, HNRF_E_ARG, "hnrf_geometry_maps: normal8 needs M");
    HNRF_REQUIRE(!depth8 || lohi, HNRF_E_ARG, "hnrf_geometry_maps: depth8 needs lohi");
    HNRF_REQUIRE(!shaded8 || N == 0 || alpha, HNRF_E_ARG, "hnrf_geometry_maps: shaded8 needs alpha");
    HNRF_REQUIRE(!offset8 || N == 0 || woff, HNRF_E_ARG, "hnrf_geometry_maps: offset8 needs woff");
    HNRF_REQUIRE(((uintptr_t)pix2ray & 3) == 0 && ((uintptr_t)normal & 3) == 0, HNRF_E_ARG,
                 "hnrf_geometry_maps: pix2ray and normal must be 4-byte aligned");
    if (!normal && !nvalid && !normal8 && !depth8 && !shaded8 && !offset8) return HNRF_OK;
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)), block(64, 4);
    hipLaunchKernelGGL(geometry_maps_kernel, grid, block, 0, (hipStream_t)stream, rays_o, rays_d, t, valid, surface, alpha, woff,
                       pix2ray, N, H, W, edge, M, bgcolor, lohi, ambient, albedo, truth8, status, normal, nvalid, normal8,
                       depth8, shaded8, offset8);
    return check_launch("hnrf_geometry_maps");
}
