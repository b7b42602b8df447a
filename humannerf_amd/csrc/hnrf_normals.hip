// Density-gradient normals (hnrf_normals.h; humannerf_amd/geometry.py holds the numpy twin of every statement here, bit
// for bit).  The gradients come from the training kernels (ops.density_gradient); this file is the HIP around them.
//
//   slot_set_kernel        one lane per kept sample: slot[idx[k]] = k (the table was cleared to -1 by a memset in front).
//   ray_normals_kernel     one wave per ray (4 per workgroup, as surface_points_kernel): lane l walks the samples l,
//                          l + 64, ...; a kept sample blends the B rotations with its bone weights (motion_Rs is read
//                          wave-uniformly: scalar loads), turns its gradient into observation space, normalises it and
//                          adds it with its compositing weight; then the xor butterfly.
//   normal_panels_kernel   one lane per pixel, 64 x 4 pixels per workgroup, lanes along x (as geometry_maps_kernel).
//   field_normals_kernel   one thread per vertex: trilinear_at for fg and the corner weights, the same coordinates once
//                          more for the derivative of the weights.
// Compiled without contraction and with the correctly rounded division and square root (Makefile).  No LDS.
#include "hnrf_common.h"
#include "hnrf_trilinear.h"

namespace hnrf {

constexpr int kNrmMaxS = 512, kNrmMaxB = 32, kNrmMaxSide = 16384, kNrmMaxG = 1024;
constexpr int64_t kNrmMaxInt = ((int64_t)1 << 31) - 1;

__device__ __forceinline__ bool nrm_finite(float v) { return fabsf(v) < __builtin_inff(); }        // (NaN: false)

__device__ __forceinline__ float nrm_len(float a, float b, float c) { return sqrtf((a * a + b * b) + c * c); }

__global__ __launch_bounds__(256) void slot_set_kernel(const int* __restrict__ idx, const int* __restrict__ count,
                                                       int64_t n_max, int64_t P, int* __restrict__ slot) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t n = *count;
    if (n > n_max) n = n_max;
    if (k >= n) return;
    const int64_t p = idx[k];
    if (p >= 0 && p < P) slot[p] = (int)k;
}

__global__ __launch_bounds__(256) void ray_normals_kernel(const float* __restrict__ weights, const float* __restrict__ bmw,
                                                          const float* __restrict__ Rs, const int* __restrict__ slot,
                                                          const float* __restrict__ g, const float* __restrict__ alpha,
                                                          int64_t R, int S, int B, float alpha_min,
                                                          float* __restrict__ normal, uint8_t* __restrict__ nvalid) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= R) return;   // wave-uniform
    const int64_t base = ray * S;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int s = lane; s < S; s += 64) {
        const int k = slot[base + s];
        if (k < 0) continue;
        const float* m = bmw + (base + s) * B;
        float A[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < B; ++b) {
            const float mb = m[b];
#pragma unroll
            for (int e = 0; e < 9; ++e) A[e] = A[e] + mb * Rs[b * 9 + e];
        }
        const float g0 = g[(int64_t)k * 3 + 0], g1 = g[(int64_t)k * 3 + 1], g2 = g[(int64_t)k * 3 + 2];
        const float v0 = -((A[0] * g0 + A[3] * g1) + A[6] * g2);
        const float v1 = -((A[1] * g0 + A[4] * g1) + A[7] * g2);
        const float v2 = -((A[2] * g0 + A[5] * g1) + A[8] * g2);
        const float len = nrm_len(v0, v1, v2);
        if (!(len > 0.f && nrm_finite(len))) continue;
        const float w = weights[base + s];
        nx = nx + w * (v0 / len);
        ny = ny + w * (v1 / len);
        nz = nz + w * (v2 / len);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        nx = nx + __shfl_xor(nx, off, 64);
        ny = ny + __shfl_xor(ny, off, 64);
        nz = nz + __shfl_xor(nz, off, 64);
    }
    if (lane != 0) return;
    const float L = nrm_len(nx, ny, nz), a = alpha[ray];
    const bool ok = nrm_finite(a) && a >= alpha_min && L > 0.f && nrm_finite(L);
    normal[ray * 3 + 0] = ok ? nx / L : 0.f;
    normal[ray * 3 + 1] = ok ? ny / L : 0.f;
    normal[ray * 3 + 2] = ok ? nz / L : 0.f;
    nvalid[ray] = ok ? 1 : 0;
}

// ---- panels
__device__ __forceinline__ uint8_t nrm_q8(float v) {
    return !(v > 0.f) ? (uint8_t)0 : v >= 1.f ? (uint8_t)255 : (uint8_t)(int)(255.f * v);
}

__device__ __forceinline__ void nrm_put3(uint8_t* __restrict__ img, int64_t pix, uint8_t a, uint8_t b, uint8_t c) {
    img[pix * 3 + 0] = a;
    img[pix * 3 + 1] = b;
    img[pix * 3 + 2] = c;
}

__global__ __launch_bounds__(256) void normal_panels_kernel(
    const float* __restrict__ rays_d, const float* __restrict__ ray_normal, const uint8_t* __restrict__ ray_nvalid,
    const uint8_t* __restrict__ valid, int bit, const float* __restrict__ alpha, const int* __restrict__ pix2ray, int64_t N,
    int H, int W, const float* __restrict__ M, const float* __restrict__ bgcolor, float ambient, float albedo,
    const int* __restrict__ status, float* __restrict__ normal, uint8_t* __restrict__ nvalid, uint8_t* __restrict__ normal8,
    uint8_t* __restrict__ shaded8) {
    if (status && *status != 0) return;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const int64_t pix = (int64_t)y * W + x;
    const int r = pix2ray[pix];
    const bool ok = r >= 0 && r < N && ((valid[r] >> bit) & 1);
    const bool has = ok && ray_nvalid[r] != 0;
    const uint8_t bg0 = nrm_q8(bgcolor[0]), bg1 = nrm_q8(bgcolor[1]), bg2 = nrm_q8(bgcolor[2]);
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (has) {
        nx = ray_normal[(int64_t)r * 3 + 0];
        ny = ray_normal[(int64_t)r * 3 + 1];
        nz = ray_normal[(int64_t)r * 3 + 2];
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
            for (int i = 0; i < 3; ++i) q[i] = nrm_q8(0.5f + 0.5f * ((M[i * 3] * nx + M[i * 3 + 1] * ny) + M[i * 3 + 2] * nz));
            nrm_put3(normal8, pix, q[0], q[1], q[2]);
        } else {
            nrm_put3(normal8, pix, bg0, bg1, bg2);
        }
    }
    if (shaded8) {
        if (ok) {
            float s = ambient;
            if (has) {
                const float d0 = rays_d[(int64_t)r * 3 + 0], d1 = rays_d[(int64_t)r * 3 + 1], d2 = rays_d[(int64_t)r * 3 + 2];
                const float nd = (nx * d0 + ny * d1) + nz * d2;
                const float dl = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
                s = ambient + (1.f - ambient) * (fabsf(nd) / dl);
            }
            const float gr = s * albedo, a = alpha[r], ga = gr * a, na = 1.f - a;
            nrm_put3(shaded8, pix, nrm_q8(ga + na * bgcolor[0]), nrm_q8(ga + na * bgcolor[1]), nrm_q8(ga + na * bgcolor[2]));
        } else {
            nrm_put3(shaded8, pix, bg0, bg1, bg2);
        }
    }
}

// ---- field normals
// One axis of trilinear_at once more: the weights u of the lower and upper node and their derivatives e with respect to
// the lattice coordinate (-1 / +1 where the node has a weight, 0 for a zero-padded node).
struct NrmAxis {
    float u[2], e[2];
};

__device__ __forceinline__ NrmAxis nrm_axis(float q, float bmin, float bscale, int G) {
    const float gm1 = (float)(G - 1);
    const float i = (((q - bmin) * bscale - 1.0f) + 1.0f) * 0.5f * gm1;
    const float f0 = floorf(i);
    const float w1 = i - f0, w0 = (f0 + 1.0f) - i;
    const int x0 = (int)fminf(fmaxf(f0, -2.0f), gm1 + 1.0f);
    const bool in0 = x0 >= 0 && x0 < G, in1 = x0 + 1 >= 0 && x0 + 1 < G;
    NrmAxis a;
    a.u[0] = in0 ? w0 : 0.f;
    a.u[1] = in1 ? w1 : 0.f;
    a.e[0] = in0 ? -1.f : 0.f;
    a.e[1] = in1 ? 1.f : 0.f;
    return a;
}

__global__ __launch_bounds__(256) void field_normals_kernel(const float* __restrict__ verts, const float* __restrict__ g,
                                                            const float* __restrict__ sigma, int64_t V,
                                                            const float* __restrict__ vol, int B, int G,
                                                            const float* __restrict__ bbox_min,
                                                            const float* __restrict__ bbox_scale, float* __restrict__ normal) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const float qx = verts[v * 3 + 0], qy = verts[v * 3 + 1], qz = verts[v * 3 + 2];
    const Trilinear t = trilinear_at(qx, qy, qz, bbox_min, bbox_scale, G);
    const NrmAxis ax = nrm_axis(qx, bbox_min[0], bbox_scale[0], G), ay = nrm_axis(qy, bbox_min[1], bbox_scale[1], G),
                  az = nrm_axis(qz, bbox_min[2], bbox_scale[2], G);
    float dcx[8], dcy[8], dcz[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = (k >> 2) & 1;
        dcx[k] = ax.e[dx] * ay.u[dy] * az.u[dz];
        dcy[k] = ax.u[dx] * ay.e[dy] * az.u[dz];
        dcz[k] = ax.u[dx] * ay.u[dy] * az.e[dz];
    }
    const size_t chan = (size_t)G * G * G;
    float fg = 0.f, Gx = 0.f, Gy = 0.f, Gz = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* ch = vol + b * chan;
        fg += trilinear_channel(t, ch);
        float wx = 0.f, wy = 0.f, wz = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float c = ch[t.o[k]];
            wx = wx + c * dcx[k];
            wy = wy + c * dcy[k];
            wz = wz + c * dcz[k];
        }
        Gx = Gx + wx;
        Gy = Gy + wy;
        Gz = Gz + wz;
    }
    const float gm1 = (float)(G - 1);
    const float fx = Gx * ((bbox_scale[0] * 0.5f) * gm1), fy = Gy * ((bbox_scale[1] * 0.5f) * gm1),
                fz = Gz * ((bbox_scale[2] * 0.5f) * gm1);
    const float sg = sigma[v];
    const bool pos = sg > 0.f;
    const float sr = pos ? sg : 0.f;
    const float g0 = pos ? g[v * 3 + 0] : 0.f, g1 = pos ? g[v * 3 + 1] : 0.f, g2 = pos ? g[v * 3 + 2] : 0.f;
    const float D0 = fg * g0 + sr * fx, D1 = fg * g1 + sr * fy, D2 = fg * g2 + sr * fz;
    const float len = nrm_len(D0, D1, D2);
    const bool ok = len > 0.f && nrm_finite(len);
    normal[v * 3 + 0] = ok ? -(D0 / len) : 0.f;
    normal[v * 3 + 1] = ok ? -(D1 / len) : 0.f;
    normal[v * 3 + 2] = ok ? -(D2 / len) : 0.f;
}

static int ray_normals_sizes_ok(int64_t R, int S) {
    return S >= 1 && S <= kNrmMaxS && R >= 0 && R * (int64_t)S <= kNrmMaxInt;
}

}  // namespace hnrf

using namespace hnrf;

extern "C" size_t hnrf_ray_normals_workspace_bytes(int64_t R, int S) {
    if (!ray_normals_sizes_ok(R, S)) return 0;
    return (size_t)R * (size_t)S * sizeof(int);
}

extern "C" int hnrf_ray_normals(const float* weights, const float* bmw, const float* motion_Rs, const int* idx,
                                const int* count, int64_t n_max, const float* g, const float* alpha, int64_t R, int S, int B,
                                float alpha_min, void* workspace, size_t workspace_bytes, float* normal, uint8_t* nvalid,
                                void* stream) {
    HNRF_REQUIRE(S >= 1, HNRF_E_ARG, "hnrf_ray_normals: S %d (1 .. %d)", S, kNrmMaxS);
    HNRF_REQUIRE(S <= kNrmMaxS, HNRF_E_UNSUPPORTED, "hnrf_ray_normals: S %d (1 .. %d)", S, kNrmMaxS);
    HNRF_REQUIRE(B >= 1, HNRF_E_ARG, "hnrf_ray_normals: B %d (1 .. %d)", B, kNrmMaxB);
    HNRF_REQUIRE(B <= kNrmMaxB, HNRF_E_UNSUPPORTED, "hnrf_ray_normals: B %d (1 .. %d)", B, kNrmMaxB);
    HNRF_REQUIRE(ray_normals_sizes_ok(R, S), HNRF_E_ARG, "hnrf_ray_normals: R %lld of S %d samples (R >= 0, R S < 2^31)",
                 (long long)R, S);
    HNRF_REQUIRE(n_max >= 0 && n_max <= kNrmMaxInt, HNRF_E_ARG, "hnrf_ray_normals: n_max %lld (0 .. 2^31 - 1)", (long long)n_max);
    HNRF_REQUIRE(alpha_min == alpha_min, HNRF_E_ARG, "hnrf_ray_normals: alpha_min is NaN");
    if (R == 0) return HNRF_OK;
    HNRF_REQUIRE(weights && bmw && motion_Rs && count && alpha, HNRF_E_ARG,
                 "hnrf_ray_normals: null pointer (weights, bmw, motion_Rs, count, alpha)");
    HNRF_REQUIRE(n_max == 0 || (idx && g), HNRF_E_ARG, "hnrf_ray_normals: null pointer (idx, g)");
    HNRF_REQUIRE(normal && nvalid, HNRF_E_ARG, "hnrf_ray_normals: null pointer (normal, nvalid)");
    HNRF_REQUIRE(workspace, HNRF_E_ARG, "hnrf_ray_normals: null pointer (workspace)");
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0, HNRF_E_ARG, "hnrf_ray_normals: workspace must be 256-byte aligned");
    const size_t need = hnrf_ray_normals_workspace_bytes(R, S);
    HNRF_REQUIRE(workspace_bytes >= need, HNRF_E_WORKSPACE, "hnrf_ray_normals: workspace of %zu bytes, %zu needed",
                 workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    int* slot = (int*)workspace;
    if (hipMemsetAsync(slot, 0xff, need, st) != hipSuccess) {
        set_error("hnrf_ray_normals: hipMemsetAsync failed");
        return HNRF_E_LAUNCH;
    }
    const int64_t P = R * (int64_t)S;
    const int64_t cap = n_max < P ? n_max : P;       // (distinct indices below P: never more than P of them)
    if (cap > 0)
        hipLaunchKernelGGL(slot_set_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, st, idx, count, cap, P, slot);
    hipLaunchKernelGGL(ray_normals_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, weights, bmw, motion_Rs,
                       (const int*)slot, g, alpha, R, S, B, alpha_min, normal, nvalid);
    return check_launch("hnrf_ray_normals");
}

extern "C" int hnrf_normal_panels(const float* rays_d, const float* ray_normal, const uint8_t* ray_nvalid,
                                  const uint8_t* valid, int surface, const float* alpha, const int* pix2ray, int64_t N, int H,
                                  int W, const float* M, const float* bgcolor, float ambient, float albedo, const int* status,
                                  float* normal, uint8_t* nvalid, uint8_t* normal8, uint8_t* shaded8, void* stream) {
    HNRF_REQUIRE(H >= 1 && H <= kNrmMaxSide, HNRF_E_ARG, "hnrf_normal_panels: H %d (1 .. %d)", H, kNrmMaxSide);
    HNRF_REQUIRE(W >= 1 && W <= kNrmMaxSide, HNRF_E_ARG, "hnrf_normal_panels: W %d (1 .. %d)", W, kNrmMaxSide);
    HNRF_REQUIRE(N >= 0 && N <= kNrmMaxInt, HNRF_E_ARG, "hnrf_normal_panels: N %lld (0 .. 2^31 - 1)", (long long)N);
    HNRF_REQUIRE(surface == 0 || surface == 1, HNRF_E_ARG, "hnrf_normal_panels: surface %d (0 = expected, 1 = median)", surface);
    HNRF_REQUIRE(ambient == ambient && albedo == albedo, HNRF_E_ARG, "hnrf_normal_panels: ambient or albedo is NaN");
    HNRF_REQUIRE(pix2ray && bgcolor, HNRF_E_ARG, "hnrf_normal_panels: null pointer (pix2ray, bgcolor)");
    HNRF_REQUIRE(N == 0 || (rays_d && ray_normal && ray_nvalid && valid), HNRF_E_ARG,
                 "hnrf_normal_panels: null pointer (rays_d, ray_normal, ray_nvalid, valid)");
    HNRF_REQUIRE(!normal8 || M, HNRF_E_ARG, "hnrf_normal_panels: normal8 needs M");
    HNRF_REQUIRE(!shaded8 || N == 0 || alpha, HNRF_E_ARG, "hnrf_normal_panels: shaded8 needs alpha");
    HNRF_REQUIRE(((uintptr_t)pix2ray & 3) == 0 && ((uintptr_t)normal & 3) == 0, HNRF_E_ARG,
                 "hnrf_normal_panels: pix2ray and normal must be 4-byte aligned");
    if (!normal && !nvalid && !normal8 && !shaded8) return HNRF_OK;
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)), block(64, 4);
    hipLaunchKernelGGL(normal_panels_kernel, grid, block, 0, (hipStream_t)stream, rays_d, ray_normal, ray_nvalid, valid, surface,
                       alpha, pix2ray, N, H, W, M, bgcolor, ambient, albedo, status, normal, nvalid, normal8, shaded8);
    return check_launch("hnrf_normal_panels");
}

extern "C" int hnrf_field_normals(const float* verts, const float* g, const float* sigma, int64_t V, const float* vol, int B,
                                  int G, const float* bbox_min, const float* bbox_scale, float* normal, void* stream) {
    HNRF_REQUIRE(V >= 0 && V <= kNrmMaxInt, HNRF_E_ARG, "hnrf_field_normals: V %lld (0 .. 2^31 - 1)", (long long)V);
    HNRF_REQUIRE(B >= 1 && B <= kNrmMaxB, HNRF_E_ARG, "hnrf_field_normals: B %d (1 .. %d)", B, kNrmMaxB);
    HNRF_REQUIRE(G >= 2 && G <= kNrmMaxG, HNRF_E_ARG, "hnrf_field_normals: G %d (2 .. %d)", G, kNrmMaxG);
    if (V == 0) return HNRF_OK;
    HNRF_REQUIRE(verts && g && sigma && vol && bbox_min && bbox_scale && normal, HNRF_E_ARG,
                 "hnrf_field_normals: null pointer (verts, g, sigma, vol, bbox_min, bbox_scale, normal)");
    hipLaunchKernelGGL(field_normals_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, g, sigma,
                       V, vol, B, G, bbox_min, bbox_scale, normal);
    return check_launch("hnrf_field_normals");
}
