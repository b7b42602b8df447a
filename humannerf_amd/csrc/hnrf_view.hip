// View-dependent colour (include/hnrf_view.h): the per-ray colour bias B e(d) + c of the folded view branch and its
// backward.  K4 / K4' with the bias are the bodies of hnrf_composite.hip / hnrf_backward.hip (a nullable pointer), the
// frame entry is in hnrf_abi.hip with the other frame entries.  No atomics: every sum here has a fixed order.
#include "hnrf_common.h"

namespace hnrf {

constexpr int kViewBandsMax = 10;
constexpr int kViewSlicesMax = 64;

// n = d / max(|d|, 1e-12) (torch.nn.functional.normalize)
__device__ __forceinline__ void view_unit(const float* __restrict__ d, float& nx, float& ny, float& nz) {
    const float dx = d[0], dy = d[1], dz = d[2];
    const float len = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
    nx = dx / len;
    ny = dy / len;
    nz = dz / len;
}

// column j of e(d) = (n, sin(2^0 n), cos(2^0 n), ...); j == E (one past the end): the constant 1 of dc
__device__ __forceinline__ float view_embed_at(float nx, float ny, float nz, int j, int E) {
    if (j >= E) return 1.f;
    const int ax = j % 3;
    const float n = ax == 0 ? nx : (ax == 1 ? ny : nz);
    if (j < 3) return n;
    const int t = (j - 3) / 3;                                    // 2 k + (0 = sin, 1 = cos)
    const float a = n * (float)(1 << (t >> 1));
    return (t & 1) ? cosf(a) : sinf(a);
}

__global__ __launch_bounds__(256) void view_bias_fwd_kernel(const float* __restrict__ dirs, const float* __restrict__ B,
                                                            const float* __restrict__ c, int L, int64_t R,
                                                            float* __restrict__ bias) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int E = 3 + 6 * L;
    float n[3];
    view_unit(dirs + r * 3, n[0], n[1], n[2]);
    const float *B0 = B, *B1 = B + E, *B2 = B + 2 * E;
    float a0 = c[0], a1 = c[1], a2 = c[2];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        a0 += B0[ax] * n[ax];
        a1 += B1[ax] * n[ax];
        a2 += B2[ax] * n[ax];
    }
    for (int k = 0; k < L; ++k) {
        const float f = (float)(1 << k);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            float sv, cv;
            sincosf(n[ax] * f, &sv, &cv);
            const int js = 3 + 6 * k + ax, jc = js + 3;
            a0 += B0[js] * sv;
            a1 += B1[js] * sv;
            a2 += B2[js] * sv;
            a0 += B0[jc] * cv;
            a1 += B1[jc] * cv;
            a2 += B2[jc] * cv;
        }
    }
    bias[r * 3 + 0] = a0;
    bias[r * 3 + 1] = a1;
    bias[r * 3 + 2] = a2;
}

// stage one: block (s, j) -> part[s][j][3] = sum over the slice's rays of d_bias[r] e_j(d_r)
__global__ __launch_bounds__(256) void view_bias_bwd_part_kernel(const float* __restrict__ dirs,
                                                                 const float* __restrict__ d_bias, int L, int64_t R,
                                                                 float* __restrict__ part) {
    const int E = 3 + 6 * L, j = blockIdx.y;
    const int64_t stride = (int64_t)gridDim.x * 256;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < R; r += stride) {
        float nx, ny, nz;
        view_unit(dirs + r * 3, nx, ny, nz);
        const float e = view_embed_at(nx, ny, nz, j, E);
        a0 += d_bias[r * 3 + 0] * e;
        a1 += d_bias[r * 3 + 1] * e;
        a2 += d_bias[r * 3 + 2] * e;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a0 += __shfl_xor(a0, off, 64);
        a1 += __shfl_xor(a1, off, 64);
        a2 += __shfl_xor(a2, off, 64);
    }
    __shared__ float red[4][3];
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = a0;
        red[threadIdx.x >> 6][1] = a1;
        red[threadIdx.x >> 6][2] = a2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float v = red[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) v += red[w][threadIdx.x];
        part[((size_t)blockIdx.x * (E + 1) + j) * 3 + threadIdx.x] = v;
    }
}

// stage two: thread (j, i) adds the slices ascending; columns j < E go to dB[i][j], column E to dc[i]
__global__ void view_bias_bwd_sum_kernel(const float* __restrict__ part, int L, int slices, float* __restrict__ dB,
                                         float* __restrict__ dc) {
    const int E = 3 + 6 * L;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (E + 1) * 3) return;
    const int j = t / 3, i = t - j * 3;
    float v = 0.f;
    for (int s = 0; s < slices; ++s) v += part[((size_t)s * (E + 1) + j) * 3 + i];
    if (j < E) dB[i * E + j] = v;
    else dc[i] = v;
}

static int view_slices(int64_t R) {
    const int64_t s = (R + 255) / 256;
    return s < 1 ? 1 : (s > kViewSlicesMax ? kViewSlicesMax : (int)s);
}

}  // namespace hnrf

using namespace hnrf;

extern "C" int hnrf_view_bias_fwd(const float* dirs, const float* B, const float* c, int L, int64_t R, float* bias,
                                  void* stream) {
    HNRF_REQUIRE(dirs && B && c && bias, HNRF_E_ARG, "hnrf_view_bias_fwd: null pointer");
    HNRF_REQUIRE(L >= 1 && L <= kViewBandsMax, HNRF_E_ARG, "hnrf_view_bias_fwd: L=%d outside 1..%d", L, kViewBandsMax);
    HNRF_REQUIRE(R >= 0, HNRF_E_ARG, "hnrf_view_bias_fwd: bad dims R=%lld", (long long)R);
    if (R == 0) return HNRF_OK;
    const int64_t blocks = (R + 255) / 256;
    HNRF_REQUIRE(blocks < (int64_t)2147483647, HNRF_E_ARG, "hnrf_view_bias_fwd: too many rays");
    hipLaunchKernelGGL(view_bias_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dirs, B, c, L, R,
                       bias);
    return check_launch("hnrf_view_bias_fwd");
}

extern "C" size_t hnrf_view_bias_bwd_workspace_bytes(int64_t R, int L) {
    if (R < 0 || L < 1 || L > kViewBandsMax) return 0;
    return align256((size_t)view_slices(R) * (size_t)(3 + 6 * L + 1) * 3 * sizeof(float));
}

extern "C" int hnrf_view_bias_bwd(const float* dirs, const float* d_bias, int L, int64_t R, void* workspace,
                                  size_t workspace_bytes, float* dB, float* dc, void* stream) {
    HNRF_REQUIRE(dirs && d_bias && dB && dc && workspace, HNRF_E_ARG, "hnrf_view_bias_bwd: null pointer");
    HNRF_REQUIRE(L >= 1 && L <= kViewBandsMax, HNRF_E_ARG, "hnrf_view_bias_bwd: L=%d outside 1..%d", L, kViewBandsMax);
    HNRF_REQUIRE(R >= 0, HNRF_E_ARG, "hnrf_view_bias_bwd: bad dims R=%lld", (long long)R);
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0, HNRF_E_ARG, "hnrf_view_bias_bwd: workspace must be 256-byte aligned");
    HNRF_REQUIRE(workspace_bytes >= hnrf_view_bias_bwd_workspace_bytes(R, L), HNRF_E_WORKSPACE,
                 "hnrf_view_bias_bwd: workspace %zu < %zu bytes", workspace_bytes, hnrf_view_bias_bwd_workspace_bytes(R, L));
    hipStream_t st = (hipStream_t)stream;
    const int E = 3 + 6 * L, slices = view_slices(R);
    // (R == 0: the one slice's loop runs no trip and writes zeros)
    hipLaunchKernelGGL(view_bias_bwd_part_kernel, dim3((unsigned)slices, (unsigned)(E + 1)), dim3(256), 0, st, dirs,
                       d_bias, L, R, (float*)workspace);
    if (int rc = check_launch("hnrf_view_bias_bwd")) return rc;
    hipLaunchKernelGGL(view_bias_bwd_sum_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, L, slices, dB, dc);
    return check_launch("hnrf_view_bias_bwd");
}
