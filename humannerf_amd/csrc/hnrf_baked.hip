// Baked canonical grid: the canonical MLP tabulated on an N^3 lattice, and the sampler that stands where K3 stands.
//
// In the configuration this library builds the canonical MLP is a pure function of the canonical position, so its
// four pre-activation outputs can be stored once per checkpoint and interpolated afterwards (an opt-in approximation).
//
// Grid: [N][N][N][4] f16, indexed [z][y][x][c], c = (r, g, b, sigma) pre-activation, 8 bytes per lattice point; the
// lattice is hnrf_density_grid's (lattice_points, hnrf_mesh.hip).  Bake: chunk by chunk the lattice positions go
// through hnrf_canonical_fwd (unchanged, every chunk range-guarded) and an epilogue converts to f16, round to nearest
// even, values beyond +-65504 (infinities included) saturated to +-65504 and counted; NaN stays NaN.
//
// Sampler (this file is compiled with -ffp-contract=off and correctly rounded division: humannerf_amd/baked.py
// restates it in numpy float32 bit for bit), per axis a with n = N - 1:
//     inv_step = (float)n / (bmax - bmin)              u = (x - bmin) * inv_step
//     u = min(max(u, 0), (float)n)                     (border replicate; max(NaN, 0) = 0)
//     i0 = min((int)floor(u), n - 1)                   t = u - (float)i0
// and with v[dz][dy][dx] the corner values converted to fp32, every channel on its own, every operation rounded on
// its own, in this order:
//     x:  c[dz][dy] = v[dz][dy][0] + tx * (v[dz][dy][1] - v[dz][dy][0])
//     y:  d[dz]     = c[dz][0] + ty * (c[dz][1] - c[dz][0])
//     z:  out       = d[0] + tz * (d[1] - d[0])
// One lane per sample, lanes along the samples of a ray (the xyz reads and raw writes stay contiguous); the two
// x-neighbours of a corner pair are 16 contiguous bytes and are fetched with one load.
//
// Baked offset field (hnrf.h "baked non-rigid offset field"): K2's offsets of ONE frame on an M^3 lattice of the same
// layout, channels (dx, dy, dz, +0), baked through hnrf_nonrigid_fwd (unchanged) and a three-channel epilogue; the
// fused sampler baked_warp_sample_kernel is sample_grid twice with one add per coordinate in between.
#include <math.h>

#include <hip/hip_fp16.h>

#include "hnrf_common.h"

namespace hnrf {
namespace {

constexpr int kThreads = 256;
constexpr float kF16Max = 65504.0f;

struct alignas(8) CornerPair {      // lattice points (x0, y, z) and (x0 + 1, y, z): 2 x 4 f16
    uint32_t w[4];
};

__device__ __forceinline__ float half_lo(uint32_t w) { return __half2float(__ushort_as_half((unsigned short)(w & 0xffffu))); }
__device__ __forceinline__ float half_hi(uint32_t w) { return __half2float(__ushort_as_half((unsigned short)(w >> 16))); }

struct Axis {
    int i0;
    float t;
};

__device__ __forceinline__ Axis axis_of(float x, float lo, float hi, int N) {
    const float n = (float)(N - 1);
    const float inv_step = n / (hi - lo);
    float u = (x - lo) * inv_step;
    u = fminf(fmaxf(u, 0.0f), n);
    Axis a;
    a.i0 = min((int)floorf(u), N - 2);
    a.t = u - (float)a.i0;
    return a;
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

__device__ __forceinline__ float4 sample_grid(const uint2* __restrict__ grid, int N, const float* __restrict__ bmin,
                                              const float* __restrict__ bmax, float x, float y, float z) {
    const Axis ax = axis_of(x, bmin[0], bmax[0], N), ay = axis_of(y, bmin[1], bmax[1], N),
               az = axis_of(z, bmin[2], bmax[2], N);
    const size_t row = (size_t)N, plane = (size_t)N * N;
    const uint2* base = grid + ((size_t)az.i0 * plane + (size_t)ay.i0 * row + (size_t)ax.i0);
    CornerPair p[2][2];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) p[dz][dy] = *(const CornerPair*)(base + dz * plane + dy * row);
    float out[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float d[2];
#pragma unroll
        for (int dz = 0; dz < 2; ++dz) {
            float e[2];
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const uint32_t w0 = p[dz][dy].w[c >> 1], w1 = p[dz][dy].w[2 + (c >> 1)];
                const float v0 = (c & 1) ? half_hi(w0) : half_lo(w0), v1 = (c & 1) ? half_hi(w1) : half_lo(w1);
                e[dy] = lerp(v0, v1, ax.t);
            }
            d[dz] = lerp(e[0], e[1], ay.t);
        }
        out[c] = lerp(d[0], d[1], az.t);
    }
    return make_float4(out[0], out[1], out[2], out[3]);
}

// idx == nullptr: sample p = the lane's index, p < P.  Else: p = idx[i] for i < *count (only those rows are read and
// written).
__global__ __launch_bounds__(kThreads) void baked_sample_kernel(const float* __restrict__ xyz,
                                                                const uint2* __restrict__ grid, int N,
                                                                const float* __restrict__ bmin,
                                                                const float* __restrict__ bmax, int64_t P,
                                                                const int* __restrict__ idx,
                                                                const int* __restrict__ count,
                                                                float4* __restrict__ raw) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int64_t p = i;
    if (idx) {
        const int64_t n = *count;
        if (i >= n || i >= P) return;
        p = idx[i];
        if (p < 0 || p >= P) return;
    } else if (i >= P) {
        return;
    }
    raw[p] = sample_grid(grid, N, bmin, bmax, xyz[3 * p + 0], xyz[3 * p + 1], xyz[3 * p + 2]);
}

__device__ __forceinline__ unsigned short to_f16_saturated(float v, int& n_sat) {
    const bool over = fabsf(v) > kF16Max;            // false for NaN
    n_sat += over ? 1 : 0;
    const float c = over ? copysignf(kF16Max, v) : v;
    return __half_as_ushort(__float2half_rn(c));
}

__global__ __launch_bounds__(kThreads) void bake_epilogue_kernel(const float4* __restrict__ raw, int64_t p0, int64_t cnt,
                                                                 uint2* __restrict__ grid,
                                                                 unsigned* __restrict__ saturated) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int n_sat = 0;
    if (i < cnt) {
        const float4 v = raw[i];
        const unsigned r = to_f16_saturated(v.x, n_sat), g = to_f16_saturated(v.y, n_sat),
                       b = to_f16_saturated(v.z, n_sat), s = to_f16_saturated(v.w, n_sat);
        grid[p0 + i] = make_uint2(r | (g << 16), b | (s << 16));
    }
    if (saturated == nullptr) return;
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) n_sat += __shfl_xor(n_sat, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && n_sat) atomicAdd(saturated, (unsigned)n_sat);
}

// Offset field of one frame, three channels: offsets [cnt,3] of K2 -> (dx, dy, dz, +0) of lattice points p0 .. p0 + cnt.
__global__ __launch_bounds__(kThreads) void bake_offsets_epilogue_kernel(const float* __restrict__ off, int64_t p0,
                                                                         int64_t cnt, uint2* __restrict__ grid,
                                                                         unsigned* __restrict__ saturated) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int n_sat = 0;
    if (i < cnt) {
        const unsigned dx = to_f16_saturated(off[3 * i + 0], n_sat), dy = to_f16_saturated(off[3 * i + 1], n_sat),
                       dz = to_f16_saturated(off[3 * i + 2], n_sat);
        grid[p0 + i] = make_uint2(dx | (dy << 16), dz);
    }
    if (saturated == nullptr) return;
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) n_sat += __shfl_xor(n_sat, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && n_sat) atomicAdd(saturated, (unsigned)n_sat);
}

// The chain baked_sample_kernel (offset grid) -> add -> baked_sample_kernel (canonical grid) for one sample per lane:
// 8 corner-pair loads of 16 B, no LDS; the offset grid's pad channel is loaded with its pair and never converted.
// xyz / offsets nullable (the lean frame writes neither); idx / count as baked_sample_kernel.
// gfx950, -O3: 40 VGPRs (as many as baked_sample_kernel: the two look-ups follow each other), 26 SGPRs, scratch
// size 0 -- nothing spills; 8 waves per SIMD.
__global__ __launch_bounds__(kThreads) void baked_warp_sample_kernel(
    const float* __restrict__ x_skel, const uint2* __restrict__ off_grid, int M, const float* __restrict__ obmin,
    const float* __restrict__ obmax, const uint2* __restrict__ grid, int N, const float* __restrict__ bmin,
    const float* __restrict__ bmax, int64_t P, const int* __restrict__ idx, const int* __restrict__ count,
    float4* __restrict__ raw, float* __restrict__ xyz, float* __restrict__ offsets) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int64_t p = i;
    if (idx) {
        const int64_t n = *count;
        if (i >= n || i >= P) return;
        p = idx[i];
        if (p < 0 || p >= P) return;
    } else if (i >= P) {
        return;
    }
    const float x = x_skel[3 * p + 0], y = x_skel[3 * p + 1], z = x_skel[3 * p + 2];
    const float4 o = sample_grid(off_grid, M, obmin, obmax, x, y, z);
    const float X = x + o.x, Y = y + o.y, Z = z + o.z;
    if (offsets) {
        offsets[3 * p + 0] = o.x;
        offsets[3 * p + 1] = o.y;
        offsets[3 * p + 2] = o.z;
    }
    if (xyz) {
        xyz[3 * p + 0] = X;
        xyz[3 * p + 1] = Y;
        xyz[3 * p + 2] = Z;
    }
    raw[p] = sample_grid(grid, N, bmin, bmax, X, Y, Z);
}

int check_grid_args(const char* who, const void* grid, int N, const float* bmin, const float* bmax) {
    HNRF_REQUIRE(grid && bmin && bmax, HNRF_E_ARG, "%s: null grid / bbox pointer", who);
    HNRF_REQUIRE(N >= 8 && N <= 512, HNRF_E_ARG, "%s: N=%d out of range [8, 512]", who, N);
    HNRF_REQUIRE(((uintptr_t)grid & 7) == 0, HNRF_E_ARG, "%s: grid must be 8-byte aligned", who);
    return HNRF_OK;
}

}  // namespace

int baked_sample(const float* xyz, const void* grid, int N, const float* bmin, const float* bmax, int64_t P,
                 const int* idx, const int* count, float* raw, hipStream_t st) {
    if (P == 0) return HNRF_OK;
    hipLaunchKernelGGL(baked_sample_kernel, dim3((unsigned)((P + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, xyz,
                       (const uint2*)grid, N, bmin, bmax, P, idx, count, (float4*)raw);
    return check_launch("hnrf_baked_sample");
}

int baked_warp_sample(const float* x_skel, const BakedGrid& off, const BakedGrid& cnl, int64_t P, const int* idx,
                      const int* count, float* raw, float* xyz, float* offsets, hipStream_t st) {
    if (P == 0) return HNRF_OK;
    hipLaunchKernelGGL(baked_warp_sample_kernel, dim3((unsigned)((P + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       x_skel, (const uint2*)off.grid, off.N, off.bmin, off.bmax, (const uint2*)cnl.grid, cnl.N, cnl.bmin,
                       cnl.bmax, P, idx, count, (float4*)raw, xyz, offsets);
    return check_launch("hnrf_baked_warp_sample");
}

}  // namespace hnrf

using namespace hnrf;

extern "C" size_t hnrf_baked_grid_bytes(int N) {
    if (N < 8 || N > 512) return 0;
    return (size_t)N * N * N * 8;
}

extern "C" size_t hnrf_bake_canonical_workspace_bytes(int N) { return hnrf_density_grid_workspace_bytes(N); }

extern "C" int hnrf_bake_canonical(const void* cnl_packed, int mode, const float* bbox_min, const float* bbox_max, int N,
                                   void* workspace, size_t workspace_bytes, void* grid, unsigned* saturated,
                                   void* stream) {
    HNRF_REQUIRE(cnl_packed && workspace, HNRF_E_ARG, "hnrf_bake_canonical: null pointer");
    int rc = check_grid_args("hnrf_bake_canonical", grid, N, bbox_min, bbox_max);
    if (rc) return rc;
    const int arith = mode & HNRF_MLP_ARITH_MASK;
    HNRF_REQUIRE(arith == HNRF_MLP_F32 || arith == HNRF_MLP_F16X3, HNRF_E_UNSUPPORTED,
                 "hnrf_bake_canonical: mode %d not built", arith);
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0, HNRF_E_ARG, "hnrf_bake_canonical: workspace must be 256-byte aligned");
    HNRF_REQUIRE(workspace_bytes >= hnrf_bake_canonical_workspace_bytes(N), HNRF_E_WORKSPACE,
                 "hnrf_bake_canonical: workspace %zu < %zu bytes", workspace_bytes, hnrf_bake_canonical_workspace_bytes(N));
    const int64_t M = (int64_t)N * N * N, C = M < kLatticeChunk ? M : kLatticeChunk;
    float* xyz = (float*)workspace;
    float* raw = (float*)((char*)workspace + align256((size_t)C * 12));
    hipStream_t st = (hipStream_t)stream;
    for (int64_t p0 = 0; p0 < M; p0 += C) {
        const int64_t cnt = (M - p0 < C) ? M - p0 : C;
        if ((rc = lattice_points(bbox_min, bbox_max, N, p0, cnt, xyz, st))) return rc;
        // every chunk guarded: a hit ORs HNRF_STATUS_F16_RANGE into the packed image's status word
        if ((rc = hnrf_canonical_fwd(xyz, cnl_packed, arith, cnt, raw, stream))) return rc;
        hipLaunchKernelGGL(bake_epilogue_kernel, dim3((unsigned)((cnt + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           (const float4*)raw, p0, cnt, (uint2*)grid, saturated);
        if ((rc = check_launch("hnrf_bake_canonical"))) return rc;
    }
    return HNRF_OK;
}

extern "C" int hnrf_baked_sample(const float* xyz, const void* grid, int N, const float* bbox_min, const float* bbox_max,
                                 int64_t P, float* raw, void* stream) {
    HNRF_REQUIRE(xyz && raw, HNRF_E_ARG, "hnrf_baked_sample: null pointer");
    int rc = check_grid_args("hnrf_baked_sample", grid, N, bbox_min, bbox_max);
    if (rc) return rc;
    HNRF_REQUIRE(P >= 0 && (P + kThreads - 1) / kThreads < 2147483647LL, HNRF_E_ARG, "hnrf_baked_sample: bad P=%lld",
                 (long long)P);
    HNRF_REQUIRE(((uintptr_t)raw & 15) == 0, HNRF_E_ARG, "hnrf_baked_sample: raw must be 16-byte aligned");
    return baked_sample(xyz, grid, N, bbox_min, bbox_max, P, nullptr, nullptr, raw, (hipStream_t)stream);
}

extern "C" int hnrf_baked_sample_sparse(const float* xyz, const void* grid, int N, const float* bbox_min,
                                        const float* bbox_max, int64_t P, const int* idx, const int* count, float* raw,
                                        void* stream) {
    HNRF_REQUIRE(xyz && raw && idx && count, HNRF_E_ARG, "hnrf_baked_sample_sparse: null pointer");
    int rc = check_grid_args("hnrf_baked_sample_sparse", grid, N, bbox_min, bbox_max);
    if (rc) return rc;
    HNRF_REQUIRE(P >= 0 && (P + kThreads - 1) / kThreads < 2147483647LL, HNRF_E_ARG,
                 "hnrf_baked_sample_sparse: bad P=%lld", (long long)P);
    HNRF_REQUIRE(((uintptr_t)raw & 15) == 0, HNRF_E_ARG, "hnrf_baked_sample_sparse: raw must be 16-byte aligned");
    return baked_sample(xyz, grid, N, bbox_min, bbox_max, P, idx, count, raw, (hipStream_t)stream);
}

extern "C" size_t hnrf_bake_nonrigid_workspace_bytes(int M) {
    if (M < 8 || M > 512) return 0;
    const int64_t L = (int64_t)M * M * M, C = L < kLatticeChunk ? L : kLatticeChunk;
    return 3 * align256((size_t)C * 12);                  // lattice positions | xyz | offsets
}

extern "C" int hnrf_bake_nonrigid(const void* nr_packed, const float* hann_w, int mode, const float* bbox_min,
                                  const float* bbox_max, int M, void* workspace, size_t workspace_bytes, void* grid,
                                  unsigned* saturated, void* stream) {
    HNRF_REQUIRE(nr_packed && hann_w && workspace, HNRF_E_ARG, "hnrf_bake_nonrigid: null pointer");
    int rc = check_grid_args("hnrf_bake_nonrigid", grid, M, bbox_min, bbox_max);
    if (rc) return rc;
    const int arith = mode & HNRF_MLP_ARITH_MASK;
    HNRF_REQUIRE(arith == HNRF_MLP_F32 || arith == HNRF_MLP_F16X3, HNRF_E_UNSUPPORTED,
                 "hnrf_bake_nonrigid: mode %d not built", arith);
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0, HNRF_E_ARG, "hnrf_bake_nonrigid: workspace must be 256-byte aligned");
    HNRF_REQUIRE(workspace_bytes >= hnrf_bake_nonrigid_workspace_bytes(M), HNRF_E_WORKSPACE,
                 "hnrf_bake_nonrigid: workspace %zu < %zu bytes", workspace_bytes, hnrf_bake_nonrigid_workspace_bytes(M));
    const int64_t L = (int64_t)M * M * M, C = L < kLatticeChunk ? L : kLatticeChunk;
    const size_t part = align256((size_t)C * 12);
    float* pts = (float*)workspace;
    float* xyz = (float*)((char*)workspace + part);
    float* off = (float*)((char*)workspace + 2 * part);
    hipStream_t st = (hipStream_t)stream;
    for (int64_t p0 = 0; p0 < L; p0 += C) {
        const int64_t cnt = (L - p0 < C) ? L - p0 : C;
        if ((rc = lattice_points(bbox_min, bbox_max, M, p0, cnt, pts, st))) return rc;
        // every chunk guarded: a hit ORs HNRF_STATUS_F16_RANGE into the packed image's status word
        if ((rc = hnrf_nonrigid_fwd(pts, hann_w, nr_packed, arith, cnt, xyz, off, stream))) return rc;
        hipLaunchKernelGGL(bake_offsets_epilogue_kernel, dim3((unsigned)((cnt + kThreads - 1) / kThreads)), dim3(kThreads),
                           0, st, (const float*)off, p0, cnt, (uint2*)grid, saturated);
        if ((rc = check_launch("hnrf_bake_nonrigid"))) return rc;
    }
    return HNRF_OK;
}

namespace {
int warp_sample_entry(const char* who, const float* x_skel, const void* off_grid, int off_M, const float* off_bbox_min,
                      const float* off_bbox_max, const void* grid, int grid_N, const float* grid_bbox_min,
                      const float* grid_bbox_max, int64_t P, const int* idx, const int* count, float* raw, float* xyz,
                      float* offsets, void* stream) {
    int rc = check_grid_args(who, off_grid, off_M, off_bbox_min, off_bbox_max);
    if (rc) return rc;
    if ((rc = check_grid_args(who, grid, grid_N, grid_bbox_min, grid_bbox_max))) return rc;
    HNRF_REQUIRE(P >= 0 && (P + kThreads - 1) / kThreads < 2147483647LL, HNRF_E_ARG, "%s: bad P=%lld", who, (long long)P);
    HNRF_REQUIRE(((uintptr_t)raw & 15) == 0, HNRF_E_ARG, "%s: raw must be 16-byte aligned", who);
    return baked_warp_sample(x_skel, BakedGrid{off_grid, off_M, off_bbox_min, off_bbox_max},
                             BakedGrid{grid, grid_N, grid_bbox_min, grid_bbox_max}, P, idx, count, raw, xyz, offsets,
                             (hipStream_t)stream);
}
}  // namespace

extern "C" int hnrf_baked_warp_sample(const float* x_skel, const void* off_grid, int off_M, const float* off_bbox_min,
                                      const float* off_bbox_max, const void* grid, int grid_N,
                                      const float* grid_bbox_min, const float* grid_bbox_max, int64_t P, float* raw,
                                      float* xyz, float* offsets, void* stream) {
    HNRF_REQUIRE(x_skel && raw, HNRF_E_ARG, "hnrf_baked_warp_sample: null pointer");
    return warp_sample_entry("hnrf_baked_warp_sample", x_skel, off_grid, off_M, off_bbox_min, off_bbox_max, grid, grid_N,
                             grid_bbox_min, grid_bbox_max, P, nullptr, nullptr, raw, xyz, offsets, stream);
}

extern "C" int hnrf_baked_warp_sample_sparse(const float* x_skel, const void* off_grid, int off_M,
                                             const float* off_bbox_min, const float* off_bbox_max, const void* grid,
                                             int grid_N, const float* grid_bbox_min, const float* grid_bbox_max, int64_t P,
                                             const int* idx, const int* count, float* raw, float* xyz, float* offsets,
                                             void* stream) {
    HNRF_REQUIRE(x_skel && raw && idx && count, HNRF_E_ARG, "hnrf_baked_warp_sample_sparse: null pointer");
    return warp_sample_entry("hnrf_baked_warp_sample_sparse", x_skel, off_grid, off_M, off_bbox_min, off_bbox_max, grid,
                             grid_N, grid_bbox_min, grid_bbox_max, P, idx, count, raw, xyz, offsets, stream);
}
