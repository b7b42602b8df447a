// LPIPS-VGG16 (hnrf.h "LPIPS"): the 13 conv3x3 + bias + ReLU layers of the VGG16 trunk as implicit GEMMs on
// v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fma chain), 2x2 max-pools, the five normalise / difference / 1x1 heads,
// and the backward with respect to the first image.  Activations are NHWC fp32.  No atomics: every sum has a fixed order.
//
// conv3x3: y[m][co] = sum_k A[m][k] Wp[co][k], m = (n, y, x) linearised, k = tap * Cin + ci (tap = 3 ky + kx), A = the
// im2col row of pixel m (zero outside the image).  Backward-data is the same product on the second packed image
// Wb[ci][tap' * Cout + co] = W[co][ci][8 - tap'] with the channel roles swapped.  Operands go through LDS in chunks of
// 32 k (one tap, 32 channels; rows of 128 B in global memory), the next chunk's global loads are in flight while the
// MFMAs of the current one run.  A lane reads four consecutive k of its row per ds_read_b128 and feeds them to four
// MFMAs; both operands use the same k permutation, so the sum is over all k in a fixed order.
// Three tilings, chosen from the layer and H*W alone (never from the batch: pair n's value cannot depend on N):
//   big128  128 pixels x 128 channels, 2x2 waves of 64x64       (>= 128 such tiles per image)
//   big64   256 pixels x  64 channels, 4x1 waves of 64x64       (>= 128 such tiles per image)
//   small    32 pixels x  32 channels, K split over the 4 waves, partial sums added through LDS as ((w0 + w1) + w2) + w3
#include "hnrf_common.h"

using namespace hnrf;

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kLayers = 13, kTaps = 5;
constexpr int kCin[kLayers] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int kCout[kLayers] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int kStage[kLayers] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};      // number of pools in front of the layer
constexpr int kTapLayer[kTaps] = {1, 3, 6, 9, 12};
constexpr int kTapC[kTaps] = {64, 128, 256, 512, 512};
constexpr int kKC = 32;        // k per chunk
constexpr int kLd = 36;        // LDS row stride in floats (144 B: 16-byte aligned rows, b128 reads spread over the banks)
__constant__ float kShift[3] = {-.030f, -.088f, -.188f};
__constant__ float kScale[3] = {.458f, .448f, .450f};

inline int fwd_K(int l) { return l == 0 ? kKC : 9 * kCin[l]; }            // 27 -> 32: zero columns
inline int bwd_rows(int l) { return l == 0 ? 32 : kCin[l]; }              // 3 -> 32: zero rows

struct PackedLayout {
    size_t wf[kLayers], wb[kLayers], bias[kLayers], head[kTaps], bytes;
};
PackedLayout packed_layout() {
    PackedLayout p;
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += align256(n); return r; };
    for (int l = 0; l < kLayers; ++l) p.wf[l] = take((size_t)kCout[l] * fwd_K(l) * 4);
    for (int l = 0; l < kLayers; ++l) p.wb[l] = take((size_t)bwd_rows(l) * 9 * kCout[l] * 4);
    for (int l = 0; l < kLayers; ++l) p.bias[l] = take((size_t)kCout[l] * 4);
    for (int t = 0; t < kTaps; ++t) p.head[t] = take((size_t)kTapC[t] * 4);
    p.bytes = o;
    return p;
}

// ---------------------------------------------------------------------------------------------------------- pack
__global__ void pack_fwd_kernel(const float* __restrict__ w, float* __restrict__ dst, int Cout, int Cin, int K) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)Cout * K) return;
    const int co = (int)(i / K), k = (int)(i % K);
    const int tap = k / Cin, ci = k % Cin;
    dst[i] = k < 9 * Cin ? w[((size_t)co * Cin + ci) * 9 + tap] : 0.f;
}
__global__ void pack_bwd_kernel(const float* __restrict__ w, float* __restrict__ dst, int rows, int Cin, int Cout) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int K = 9 * Cout;
    if (i >= (int64_t)rows * K) return;
    const int ci = (int)(i / K), k = (int)(i % K);
    const int tap = k / Cout, co = k % Cout;
    dst[i] = ci < Cin ? w[((size_t)co * Cin + ci) * 9 + (8 - tap)] : 0.f;
}
__global__ void copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------------------- conv3x3
struct ConvArgs {
    const float* x;        // [N,H,W,Cin]; FIRST: images [.,H,W,3] of the pairs' first members
    const float* x1;       // FIRST: images of n >= nsplit (null: all from x)
    const float* mask;     // nullable, x's shape: x counts only where mask > 0
    const float* w;        // packed [rows][K]
    const float* bias;     // [Cout]: y = max(acc + bias, 0); null: y = acc
    float* y;              // [N,H,W,Cout]
    int N, H, W, Cin, Cout, K, nsplit;
    int scale_in;          // FIRST: (x - shift) / scale on in-range pixels
    int unscale_out;       // y / scale[co]
};

template <int WM, int WN, bool SPLITK, bool FIRST>
__global__ __launch_bounds__(256) void conv3x3_kernel(ConvArgs a) {
    constexpr int T = SPLITK ? 1 : 2;                       // 32x32 tiles per wave in each direction
    constexpr int BM = SPLITK ? 32 : WM * 64, BN = SPLITK ? 32 : WN * 64;
    constexpr int AROWS = SPLITK ? 128 : BM, BROWS = SPLITK ? 128 : BN;      // split-K: a slab per wave
    constexpr int LT = SPLITK ? 64 : 256;                   // threads that load one slab together
    constexpr int NA = BM * 8 / LT, NB = BN * 8 / LT;       // float4 per thread and chunk
    __shared__ __attribute__((aligned(16))) float As[AROWS * kLd];
    __shared__ __attribute__((aligned(16))) float Bs[BROWS * kLd];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lt = SPLITK ? lane : tid;
    const int slab = SPLITK ? wave * 32 : 0;
    const int M = a.N * a.H * a.W, HW = a.H * a.W;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

    // the im2col rows this thread loads: pixel coordinates and the address of the pixel's channel vector
    int py[NA], px[NA];
    const float* prow[NA];
    const float* pmask[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int row = (lt + i * LT) >> 3, m = m0 + row;
        py[i] = -0x10000; px[i] = -0x10000; prow[i] = a.x; pmask[i] = a.mask;
        if (m < M) {
            const int n = m / HW, r = m - n * HW;
            py[i] = r / a.W;
            px[i] = r - py[i] * a.W;
            if (FIRST && a.x1 != nullptr && n >= a.nsplit) prow[i] = a.x1 + ((size_t)m - (size_t)a.nsplit * HW) * a.Cin;
            else prow[i] = a.x + (size_t)m * a.Cin;
            if (a.mask) pmask[i] = a.mask + (size_t)m * a.Cin;
        }
    }
    const float* wrow[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) wrow[i] = a.w + (size_t)(n0 + ((lt + i * LT) >> 3)) * a.K + ((lt + i * LT) & 7) * 4;

    float4 ra[NA], rb[NB];
    auto load = [&](int ch) {
        const int k0 = ch * kKC;
        if (FIRST) {                                        // Cin = 3: the whole K in one chunk, element by element
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int q = (lt + i * LT) & 7;
                float v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int k = k0 + q * 4 + c, tap = k / a.Cin, ci = k - tap * a.Cin;
                    const int yy = py[i] + tap / 3 - 1, xx = px[i] + tap % 3 - 1;
                    v[c] = 0.f;
                    if (tap < 9 && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
                        const float t = prow[i][((tap / 3 - 1) * a.W + (tap % 3 - 1)) * a.Cin + ci];
                        v[c] = a.scale_in ? (t - kShift[ci % 3]) / kScale[ci % 3] : t;
                    }
                }
                ra[i] = make_float4(v[0], v[1], v[2], v[3]);
            }
        } else {
            const int tap = k0 / a.Cin, ci0 = k0 - tap * a.Cin, dy = tap / 3 - 1, dx = tap % 3 - 1;
            const int off = (dy * a.W + dx) * a.Cin + ci0;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int q = (lt + i * LT) & 7, yy = py[i] + dy, xx = px[i] + dx;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
                    v = *reinterpret_cast<const float4*>(prow[i] + off + q * 4);
                    if (a.mask) {
                        const float4 mk = *reinterpret_cast<const float4*>(pmask[i] + off + q * 4);
                        v.x = mk.x > 0.f ? v.x : 0.f;
                        v.y = mk.y > 0.f ? v.y : 0.f;
                        v.z = mk.z > 0.f ? v.z : 0.f;
                        v.w = mk.w > 0.f ? v.w : 0.f;
                    }
                }
                ra[i] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) rb[i] = *reinterpret_cast<const float4*>(wrow[i] + k0);
    };

    f32x16 acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nch = a.K / kKC;
    const int nloc = SPLITK ? (nch + 3) / 4 : nch;          // chunks per wave; the same trip count for every wave
    const int cbase = SPLITK ? wave * nloc : 0;
    const int arow = (SPLITK ? slab : (wave / WN) * 64) + (lane & 31);
    const int brow = (SPLITK ? slab : (wave % WN) * 64) + (lane & 31);
    const int kh = (lane >> 5) * 4;

    if (cbase < nch) load(cbase);
    for (int c = 0; c < nloc; ++c) {
        const bool valid = cbase + c < nch;                 // wave-uniform
        if (valid) {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int idx = lt + i * LT;
                *reinterpret_cast<float4*>(&As[(slab + (idx >> 3)) * kLd + (idx & 7) * 4]) = ra[i];
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int idx = lt + i * LT;
                *reinterpret_cast<float4*>(&Bs[(slab + (idx >> 3)) * kLd + (idx & 7) * 4]) = rb[i];
            }
        }
        __syncthreads();
        if (c + 1 < nloc && cbase + c + 1 < nch) load(cbase + c + 1);
        if (valid) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float4 av[T], bv[T];
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    av[t] = *reinterpret_cast<const float4*>(&As[(arow + t * 32) * kLd + s * 8 + kh]);
                    bv[t] = *reinterpret_cast<const float4*>(&Bs[(brow + t * 32) * kLd + s * 8 + kh]);
                }
#pragma unroll
                for (int i = 0; i < T; ++i)
#pragma unroll
                    for (int j = 0; j < T; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].x, bv[j].x, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].y, bv[j].y, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].z, bv[j].z, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].w, bv[j].w, acc[i][j], 0, 0, 0);
                    }
            }
        }
        __syncthreads();
    }

    if (SPLITK) {                                           // ((w0 + w1) + w2) + w3 through the A slab
        if (wave > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) As[(wave - 1) * 1024 + r * 64 + lane] = acc[0][0][r];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc[0][0][r] = ((acc[0][0][r] + As[r * 64 + lane]) + As[1024 + r * 64 + lane]) + As[2048 + r * 64 + lane];
    }

    const int mw = m0 + (SPLITK ? 0 : (wave / WN) * 64), nw = n0 + (SPLITK ? 0 : (wave % WN) * 64);
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int co = nw + j * 32 + (lane & 31);
            if (co >= a.Cout) continue;
            const float b = a.bias ? a.bias[co] : 0.f;
            const float sc = a.unscale_out ? kScale[co % 3] : 1.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mw + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m >= M) continue;
                float v = acc[i][j][r];
                if (a.bias) v = fmaxf(v + b, 0.f);
                if (a.unscale_out) v = v / sc;
                a.y[(size_t)m * a.Cout + co] = v;
            }
        }
}

// rows: the packed image's (padded) row count; the tiling depends on the layer and H*W only
int launch_conv(const char* who, const ConvArgs& a, int rows, bool first, hipStream_t st) {
    const int64_t M = (int64_t)a.N * a.H * a.W, HW = (int64_t)a.H * a.W;
    if (M == 0) return HNRF_OK;
    if (first) {
        hipLaunchKernelGGL((conv3x3_kernel<1, 1, true, true>), dim3((unsigned)((M + 31) / 32), rows / 32), dim3(256), 0, st, a);
    } else if (rows % 128 == 0 && ((HW + 127) / 128) * (rows / 128) >= 128) {
        hipLaunchKernelGGL((conv3x3_kernel<2, 2, false, false>), dim3((unsigned)((M + 127) / 128), rows / 128), dim3(256), 0, st, a);
    } else if (rows % 64 == 0 && ((HW + 255) / 256) * (rows / 64) >= 128) {
        hipLaunchKernelGGL((conv3x3_kernel<4, 1, false, false>), dim3((unsigned)((M + 255) / 256), rows / 64), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((conv3x3_kernel<1, 1, true, false>), dim3((unsigned)((M + 31) / 32), rows / 32), dim3(256), 0, st, a);
    }
    return check_launch(who);
}

int check_image_dims(const char* who, int N, int H, int W, int C) {
    HNRF_REQUIRE(N >= 0 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, HNRF_E_UNSUPPORTED, "%s: bad dims N=%d H=%d W=%d", who, N, H, W);
    HNRF_REQUIRE((int64_t)N * H * W * C < ((int64_t)1 << 31), HNRF_E_UNSUPPORTED,
                 "%s: N*H*W*C = %lld does not fit 31 bits", who, (long long)((int64_t)N * H * W * C));
    return HNRF_OK;
}

int conv_fwd(const char* who, const float* x, const float* x1, int nsplit, const void* packed, int l, int N, int H, int W,
             int scale_in, float* y, hipStream_t st) {
    const PackedLayout p = packed_layout();
    ConvArgs a{x, x1, nullptr, (const float*)((const char*)packed + p.wf[l]), (const float*)((const char*)packed + p.bias[l]),
               y, N, H, W, kCin[l], kCout[l], fwd_K(l), nsplit, scale_in, 0};
    return launch_conv(who, a, kCout[l], l == 0, st);
}
int conv_bwd(const char* who, const float* dy, const float* y_saved, const void* packed, int l, int N, int H, int W,
             int unscale_out, float* dx, hipStream_t st) {
    const PackedLayout p = packed_layout();
    ConvArgs a{dy, nullptr, y_saved, (const float*)((const char*)packed + p.wb[l]), nullptr,
               dx, N, H, W, kCout[l], kCin[l], 9 * kCout[l], 0, 0, unscale_out};
    return launch_conv(who, a, bwd_rows(l), false, st);
}

// ---------------------------------------------------------------------------------------------------------- maxpool2
__global__ void maxpool2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // over [N,Ho,Wo,C/4]
    if (i >= total) return;
    const int Ho = H >> 1, Wo = W >> 1, C4 = C >> 2;
    const int c = (int)(i % C4);
    int64_t r = i / C4;
    const int xo = (int)(r % Wo); r /= Wo;
    const int yo = (int)(r % Ho);
    const int64_t n = r / Ho;
    const float4* p = reinterpret_cast<const float4*>(x + ((n * H + 2 * yo) * W + 2 * xo) * C) + c;
    const float4 v0 = p[0], v1 = p[C4], v2 = p[(size_t)W * C4], v3 = p[(size_t)W * C4 + C4];
    float4 o;
    o.x = fmaxf(fmaxf(v0.x, v1.x), fmaxf(v2.x, v3.x));
    o.y = fmaxf(fmaxf(v0.y, v1.y), fmaxf(v2.y, v3.y));
    o.z = fmaxf(fmaxf(v0.z, v1.z), fmaxf(v2.z, v3.z));
    o.w = fmaxf(fmaxf(v0.w, v1.w), fmaxf(v2.w, v3.w));
    reinterpret_cast<float4*>(y)[i] = o;
}

// the gradient goes to the first maximum of the window in row-major scan order
__device__ inline float route(float dy, float v0, float v1, float v2, float v3, int me) {
    int best = 0;
    float bv = v0;
    if (v1 > bv) { bv = v1; best = 1; }
    if (v2 > bv) { bv = v2; best = 2; }
    if (v3 > bv) { bv = v3; best = 3; }
    return best == me ? dy : 0.f;
}
__global__ void maxpool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int H,
                                    int W, int C, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // over [N,H,W,C/4]
    if (i >= total) return;
    const int Ho = H >> 1, Wo = W >> 1, C4 = C >> 2;
    const int c = (int)(i % C4);
    int64_t r = i / C4;
    const int xi = (int)(r % W); r /= W;
    const int yi = (int)(r % H);
    const int64_t n = r / H;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    const int yo = yi >> 1, xo = xi >> 1;
    if (yo < Ho && xo < Wo) {                               // floor mode: an odd last row / column belongs to no window
        const float4* p = reinterpret_cast<const float4*>(x + ((n * H + 2 * yo) * W + 2 * xo) * C) + c;
        const float4 v0 = p[0], v1 = p[C4], v2 = p[(size_t)W * C4], v3 = p[(size_t)W * C4 + C4];
        const float4 g = reinterpret_cast<const float4*>(dy + ((n * Ho + yo) * Wo + xo) * C)[c];
        const int me = (yi & 1) * 2 + (xi & 1);
        o.x = route(g.x, v0.x, v1.x, v2.x, v3.x, me);
        o.y = route(g.y, v0.y, v1.y, v2.y, v3.y, me);
        o.z = route(g.z, v0.z, v1.z, v2.z, v3.z, me);
        o.w = route(g.w, v0.w, v1.w, v2.w, v3.w, me);
    }
    reinterpret_cast<float4*>(dx)[i] = o;
}

// ---------------------------------------------------------------------------------------------------------- heads
__device__ inline float wave_sum(float v) {                 // fixed butterfly: every lane gets the same bits
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave per pixel of one pair: pix[n P + p] = sum_c w_c (x0_c / d0 - x1_c / d1)^2, d = sqrt(sum x^2 + 1e-10) + 1e-10
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ f, const float* __restrict__ w, int N,
                                                       int64_t P, int C, float* __restrict__ pix) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= N * P) return;
    const float* f0 = f + q * C;
    const float* f1 = f + (N * P + q) * C;
    const int nI = C >> 6;
    float x0[8], x1[8], s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x0[i] = 0.f; x1[i] = 0.f;
        if (i < nI) {
            x0[i] = f0[lane + 64 * i];
            x1[i] = f1[lane + 64 * i];
            s0 = fmaf(x0[i], x0[i], s0);
            s1 = fmaf(x1[i], x1[i], s1);
        }
    }
    const float d0 = sqrtf(wave_sum(s0) + 1e-10f) + 1e-10f, d1 = sqrtf(wave_sum(s1) + 1e-10f) + 1e-10f;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < nI) {
            const float e = x0[i] / d0 - x1[i] / d1;
            t = fmaf(w[lane + 64 * i] * e, e, t);
        }
    t = wave_sum(t);
    if (lane == 0) pix[q] = t;
}

// one block per pair: the spatial mean in a fixed order (thread t sums p = t, t + 256, ... in fp64, then a tree)
__global__ __launch_bounds__(256) void head_mean_kernel(const float* __restrict__ pix, int64_t P, float* __restrict__ out,
                                                        int accumulate, float* __restrict__ layer_val) {
    __shared__ double red[256];
    const int n = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int64_t p = t; p < P; p += 256) s += (double)pix[n * P + p];
    red[t] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) {
        const float v = (float)(red[0] / (double)P);
        out[n] = accumulate ? out[n] + v : v;
        if (layer_val) layer_val[n] = v;
    }
}

// dx0_k = go / P * ( q_k / d0 - (sum_c q_c x0_c) x0_k / (d0^2 sqrt(s0 + 1e-10)) ),  q_c = 2 w_c (x0_c / d0 - x1_c / d1)
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ f, const float* __restrict__ w,
                                                       const float* __restrict__ go, int N, int64_t P, int C,
                                                       float* __restrict__ dx, int accumulate) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= N * P) return;
    const float* f0 = f + q * C;
    const float* f1 = f + (N * P + q) * C;
    float* g = dx + q * C;
    const int nI = C >> 6;
    float x0[8], x1[8], s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x0[i] = 0.f; x1[i] = 0.f;
        if (i < nI) {
            x0[i] = f0[lane + 64 * i];
            x1[i] = f1[lane + 64 * i];
            s0 = fmaf(x0[i], x0[i], s0);
            s1 = fmaf(x1[i], x1[i], s1);
        }
    }
    const float r0 = sqrtf(wave_sum(s0) + 1e-10f), d0 = r0 + 1e-10f, d1 = sqrtf(wave_sum(s1) + 1e-10f) + 1e-10f;
    float qv[8], dot = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        qv[i] = 0.f;
        if (i < nI) {
            qv[i] = 2.f * w[lane + 64 * i] * (x0[i] / d0 - x1[i] / d1);
            dot = fmaf(qv[i], x0[i], dot);
        }
    }
    dot = wave_sum(dot);
    const float up = go[q / P] / (float)P, k2 = dot / (d0 * d0 * r0);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < nI) {
            const float v = up * (qv[i] / d0 - k2 * x0[i]);
            g[lane + 64 * i] = accumulate ? g[lane + 64 * i] + v : v;
        }
}

bool head_channels_ok(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }

// ---------------------------------------------------------------------------------------------------------- workspace
// want_grad: y[13] (both image sets, 2N images) | pool[4] | g[2] (N images, 64 channels at full size) | pix[N H W]
// else:      buf[2] (2N images, 64 channels at full size) | pix
struct LpipsCarve {
    float *y[kLayers], *pool[4], *g[2], *buf[2], *pix;
    size_t bytes;
};
LpipsCarve lpips_carve(void* base, int N, int H, int W, int want_grad) {
    LpipsCarve c{};
    size_t o = 0;
    auto take = [&](size_t nfloat) {
        float* p = (float*)((uintptr_t)base + o);
        o += align256(nfloat * 4);
        return p;
    };
    const size_t B = 2 * (size_t)N;
    if (want_grad) {
        for (int l = 0; l < kLayers; ++l) c.y[l] = take(B * (H >> kStage[l]) * (W >> kStage[l]) * kCout[l]);
        for (int s = 1; s <= 4; ++s) c.pool[s - 1] = take(B * (H >> s) * (W >> s) * kTapC[s - 1]);
        for (int i = 0; i < 2; ++i) c.g[i] = take((size_t)N * H * W * 64);
    } else {
        for (int i = 0; i < 2; ++i) c.buf[i] = take(B * H * W * 64);
    }
    c.pix = take((size_t)N * H * W);
    c.bytes = o;
    return c;
}

int check_lpips_dims(const char* who, int N, int H, int W) {
    HNRF_REQUIRE(N >= 0, HNRF_E_UNSUPPORTED, "%s: N=%d", who, N);
    HNRF_REQUIRE(H >= 16 && W >= 16, HNRF_E_UNSUPPORTED, "%s: H=%d W=%d below 16 (four 2x2 pools)", who, H, W);
    return check_image_dims(who, 2 * N, H, W, 64);
}

int pool_fwd(const char* who, const float* x, int N, int H, int W, int C, float* y, hipStream_t st) {
    const int64_t total = (int64_t)N * (H >> 1) * (W >> 1) * (C >> 2);
    if (total == 0) return HNRF_OK;
    hipLaunchKernelGGL(maxpool2_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, y, H, W, C, total);
    return check_launch(who);
}
int pool_bwd(const char* who, const float* x, const float* dy, int N, int H, int W, int C, float* dx, hipStream_t st) {
    const int64_t total = (int64_t)N * H * W * (C >> 2);
    if (total == 0) return HNRF_OK;
    hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, dy, dx, H, W, C, total);
    return check_launch(who);
}
int head_fwd(const char* who, const float* f, const float* w, int N, int64_t P, int C, float* pix, float* out, int accumulate,
             float* layer_val, hipStream_t st) {
    if (N == 0) return HNRF_OK;
    hipLaunchKernelGGL(head_fwd_kernel, dim3((unsigned)((N * P + 3) / 4)), dim3(256), 0, st, f, w, N, P, C, pix);
    hipLaunchKernelGGL(head_mean_kernel, dim3(N), dim3(256), 0, st, (const float*)pix, P, out, accumulate, layer_val);
    return check_launch(who);
}
int head_bwd(const char* who, const float* f, const float* w, const float* go, int N, int64_t P, int C, float* dx,
             int accumulate, hipStream_t st) {
    if (N == 0) return HNRF_OK;
    hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)((N * P + 3) / 4)), dim3(256), 0, st, f, w, go, N, P, C, dx, accumulate);
    return check_launch(who);
}
}  // namespace

// ------------------------------------------------------------------------------------------------------------ C ABI
extern "C" size_t hnrf_lpips_packed_bytes(void) { return packed_layout().bytes; }

extern "C" int hnrf_lpips_pack(const float* const* w, const float* const* b, const float* const* lin, void* packed,
                               void* stream) {
    HNRF_REQUIRE(w && b && lin && packed, HNRF_E_ARG, "hnrf_lpips_pack: null pointer");
    for (int l = 0; l < kLayers; ++l) HNRF_REQUIRE(w[l] && b[l], HNRF_E_ARG, "hnrf_lpips_pack: null pointer (conv %d)", l);
    for (int t = 0; t < kTaps; ++t) HNRF_REQUIRE(lin[t], HNRF_E_ARG, "hnrf_lpips_pack: null pointer (head %d)", t);
    HNRF_REQUIRE(((uintptr_t)packed & 255) == 0, HNRF_E_ARG, "hnrf_lpips_pack: packed must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const PackedLayout p = packed_layout();
    char* base = (char*)packed;
    for (int l = 0; l < kLayers; ++l) {
        const int64_t nf = (int64_t)kCout[l] * fwd_K(l), nb = (int64_t)bwd_rows(l) * 9 * kCout[l];
        hipLaunchKernelGGL(pack_fwd_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, w[l], (float*)(base + p.wf[l]),
                           kCout[l], kCin[l], fwd_K(l));
        hipLaunchKernelGGL(pack_bwd_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, w[l], (float*)(base + p.wb[l]),
                           bwd_rows(l), kCin[l], kCout[l]);
        hipLaunchKernelGGL(copy_kernel, dim3((kCout[l] + 255) / 256), dim3(256), 0, st, b[l], (float*)(base + p.bias[l]), kCout[l]);
    }
    for (int t = 0; t < kTaps; ++t)
        hipLaunchKernelGGL(copy_kernel, dim3((kTapC[t] + 255) / 256), dim3(256), 0, st, lin[t], (float*)(base + p.head[t]), kTapC[t]);
    return check_launch("hnrf_lpips_pack");
}

extern "C" int hnrf_conv3x3_fwd(const float* x, const void* packed, int layer, int N, int H, int W, int scale_input, float* y,
                                void* stream) {
    HNRF_REQUIRE(x && packed && y, HNRF_E_ARG, "hnrf_conv3x3_fwd: null pointer");
    HNRF_REQUIRE(layer >= 0 && layer < kLayers, HNRF_E_UNSUPPORTED, "hnrf_conv3x3_fwd: layer %d not in 0..12", layer);
    HNRF_REQUIRE(!scale_input || layer == 0, HNRF_E_UNSUPPORTED, "hnrf_conv3x3_fwd: the scaling layer goes with layer 0");
    if (int rc = check_image_dims("hnrf_conv3x3_fwd", N, H, W, kCout[layer])) return rc;
    HNRF_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)packed) & 15) == 0, HNRF_E_ARG, "hnrf_conv3x3_fwd: pointers must be 16-byte aligned");
    return conv_fwd("hnrf_conv3x3_fwd", x, nullptr, 0, packed, layer, N, H, W, scale_input, y, (hipStream_t)stream);
}

extern "C" int hnrf_conv3x3_bwd_data(const float* dy, const float* y_saved, const void* packed, int layer, int N, int H, int W,
                                     int unscale_output, float* dx, void* stream) {
    HNRF_REQUIRE(dy && packed && dx, HNRF_E_ARG, "hnrf_conv3x3_bwd_data: null pointer");
    HNRF_REQUIRE(layer >= 0 && layer < kLayers, HNRF_E_UNSUPPORTED, "hnrf_conv3x3_bwd_data: layer %d not in 0..12", layer);
    HNRF_REQUIRE(!unscale_output || layer == 0, HNRF_E_UNSUPPORTED, "hnrf_conv3x3_bwd_data: the scaling layer goes with layer 0");
    if (int rc = check_image_dims("hnrf_conv3x3_bwd_data", N, H, W, kCout[layer])) return rc;
    HNRF_REQUIRE((((uintptr_t)dy | (uintptr_t)y_saved | (uintptr_t)dx | (uintptr_t)packed) & 15) == 0, HNRF_E_ARG,
                 "hnrf_conv3x3_bwd_data: pointers must be 16-byte aligned");
    return conv_bwd("hnrf_conv3x3_bwd_data", dy, y_saved, packed, layer, N, H, W, unscale_output, dx, (hipStream_t)stream);
}

extern "C" int hnrf_maxpool2_fwd(const float* x, int N, int H, int W, int C, float* y, void* stream) {
    HNRF_REQUIRE(x && y, HNRF_E_ARG, "hnrf_maxpool2_fwd: null pointer");
    HNRF_REQUIRE(C >= 4 && C % 4 == 0, HNRF_E_UNSUPPORTED, "hnrf_maxpool2_fwd: C=%d is no multiple of 4", C);
    if (int rc = check_image_dims("hnrf_maxpool2_fwd", N, H, W, C)) return rc;
    HNRF_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, HNRF_E_ARG, "hnrf_maxpool2_fwd: pointers must be 16-byte aligned");
    return pool_fwd("hnrf_maxpool2_fwd", x, N, H, W, C, y, (hipStream_t)stream);
}

extern "C" int hnrf_maxpool2_bwd(const float* x, const float* dy, int N, int H, int W, int C, float* dx, void* stream) {
    HNRF_REQUIRE(x && dy && dx, HNRF_E_ARG, "hnrf_maxpool2_bwd: null pointer");
    HNRF_REQUIRE(C >= 4 && C % 4 == 0, HNRF_E_UNSUPPORTED, "hnrf_maxpool2_bwd: C=%d is no multiple of 4", C);
    if (int rc = check_image_dims("hnrf_maxpool2_bwd", N, H, W, C)) return rc;
    HNRF_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0, HNRF_E_ARG, "hnrf_maxpool2_bwd: pointers must be 16-byte aligned");
    return pool_bwd("hnrf_maxpool2_bwd", x, dy, N, H, W, C, dx, (hipStream_t)stream);
}

extern "C" int hnrf_lpips_head_fwd(const float* f, const float* w, int N, int64_t P, int C, float* pix_ws, float* out,
                                   int accumulate, float* layer_val, void* stream) {
    HNRF_REQUIRE(f && w && pix_ws && out, HNRF_E_ARG, "hnrf_lpips_head_fwd: null pointer");
    HNRF_REQUIRE(head_channels_ok(C), HNRF_E_UNSUPPORTED, "hnrf_lpips_head_fwd: C=%d not in {64, 128, 256, 512}", C);
    HNRF_REQUIRE(N >= 0 && P >= 1 && 2 * (int64_t)N * P * C < ((int64_t)1 << 40), HNRF_E_UNSUPPORTED, "hnrf_lpips_head_fwd: bad dims");
    return head_fwd("hnrf_lpips_head_fwd", f, w, N, P, C, pix_ws, out, accumulate, layer_val, (hipStream_t)stream);
}

extern "C" int hnrf_lpips_head_bwd(const float* f, const float* w, const float* grad_out, int N, int64_t P, int C, float* dx,
                                   int accumulate, void* stream) {
    HNRF_REQUIRE(f && w && grad_out && dx, HNRF_E_ARG, "hnrf_lpips_head_bwd: null pointer");
    HNRF_REQUIRE(head_channels_ok(C), HNRF_E_UNSUPPORTED, "hnrf_lpips_head_bwd: C=%d not in {64, 128, 256, 512}", C);
    HNRF_REQUIRE(N >= 0 && P >= 1 && 2 * (int64_t)N * P * C < ((int64_t)1 << 40), HNRF_E_UNSUPPORTED, "hnrf_lpips_head_bwd: bad dims");
    return head_bwd("hnrf_lpips_head_bwd", f, w, grad_out, N, P, C, dx, accumulate, (hipStream_t)stream);
}

extern "C" size_t hnrf_lpips_workspace_bytes(int N, int H, int W, int want_grad) {
    if (N < 0 || H < 16 || W < 16 || H > 32768 || W > 32768 || (int64_t)2 * N * H * W * 64 >= ((int64_t)1 << 31)) return 0;
    return lpips_carve(nullptr, N, H, W, want_grad).bytes;
}

extern "C" int hnrf_lpips_fwd(const float* img0, const float* img1, const void* packed, int N, int H, int W, int want_grad,
                              void* workspace, size_t workspace_bytes, float* out, float* per_layer, void* stream) {
    const char* who = "hnrf_lpips_fwd";
    HNRF_REQUIRE(img0 && img1 && packed && workspace && out, HNRF_E_ARG, "%s: null pointer", who);
    if (int rc = check_lpips_dims(who, N, H, W)) return rc;
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)packed & 255) == 0, HNRF_E_ARG,
                 "%s: workspace and packed must be 256-byte aligned", who);
    const LpipsCarve c = lpips_carve(workspace, N, H, W, want_grad);
    HNRF_REQUIRE(workspace_bytes >= c.bytes, HNRF_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, c.bytes);
    if (N == 0) return HNRF_OK;
    hipStream_t st = (hipStream_t)stream;
    const PackedLayout p = packed_layout();
    const int B = 2 * N;
    const float* cur = nullptr;
    int flip = 0, rc;
    for (int l = 0; l < kLayers; ++l) {
        const int s = kStage[l], h = H >> s, w = W >> s;
        if (l > 0 && kStage[l - 1] != s) {                  // 2x2 pool in front of this layer
            float* dst = want_grad ? c.pool[s - 1] : c.buf[flip ^= 1];
            if ((rc = pool_fwd(who, cur, B, H >> (s - 1), W >> (s - 1), kCin[l], dst, st))) return rc;
            cur = dst;
        }
        float* y = want_grad ? c.y[l] : c.buf[flip ^= 1];
        rc = l == 0 ? conv_fwd(who, img0, img1, N, packed, 0, B, h, w, 1, y, st)
                    : conv_fwd(who, cur, nullptr, 0, packed, l, B, h, w, 0, y, st);
        if (rc) return rc;
        cur = y;
        for (int t = 0; t < kTaps; ++t)
            if (kTapLayer[t] == l &&
                (rc = head_fwd(who, cur, (const float*)((const char*)packed + p.head[t]), N, (int64_t)h * w, kTapC[t], c.pix,
                               out, t > 0, per_layer ? per_layer + (size_t)t * N : nullptr, st)))
                return rc;
    }
    return HNRF_OK;
}

extern "C" int hnrf_lpips_bwd(const float* grad_out, const void* packed, int N, int H, int W, void* workspace,
                              size_t workspace_bytes, float* d_img0, void* stream) {
    const char* who = "hnrf_lpips_bwd";
    HNRF_REQUIRE(grad_out && packed && workspace && d_img0, HNRF_E_ARG, "%s: null pointer", who);
    if (int rc = check_lpips_dims(who, N, H, W)) return rc;
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)packed & 255) == 0, HNRF_E_ARG,
                 "%s: workspace and packed must be 256-byte aligned", who);
    const LpipsCarve c = lpips_carve(workspace, N, H, W, 1);
    HNRF_REQUIRE(workspace_bytes >= c.bytes, HNRF_E_WORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, c.bytes);
    if (N == 0) return HNRF_OK;
    hipStream_t st = (hipStream_t)stream;
    const PackedLayout p = packed_layout();
    float* g = nullptr;                                     // gradient at the output of the layer being processed
    int flip = 0, rc;
    for (int t = kTaps - 1; t >= 0; --t) {
        const int L = kTapLayer[t], h = H >> t, w = W >> t;
        float* gt = c.g[flip ^= 1];
        if (t < kTaps - 1 && (rc = pool_bwd(who, c.y[L], g, N, h, w, kTapC[t], gt, st))) return rc;
        if ((rc = head_bwd(who, c.y[L], (const float*)((const char*)packed + p.head[t]), grad_out, N, (int64_t)h * w, kTapC[t],
                           gt, t < kTaps - 1, st)))
            return rc;
        g = gt;
        for (int l = L; l >= 0 && kStage[l] == t; --l) {
            float* dx = l == 0 ? d_img0 : c.g[flip ^= 1];
            if ((rc = conv_bwd(who, g, c.y[l], packed, l, N, h, w, l == 0, dx, st))) return rc;
            g = dx;
        }
    }
    return HNRF_OK;
}
