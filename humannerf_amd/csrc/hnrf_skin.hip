// Bone weights as data and the skinning of a glTF viewer (include/hnrf_skin.h): the device side of the skinned glTF
// export.  One thread per vertex, memory-bound, no atomics.  Compiled with -ffp-contract=off and IEEE division: every
// operation is rounded on its own, in the order the header states, and humannerf_amd/skin.py restates both kernels in
// numpy float32 bit for bit.  The bone weight is hnrf_forward_skin's own device function (hnrf_trilinear.h).
#include "hnrf_trilinear.h"

namespace hnrf {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxSkinBones = 128;

// K slots in registers (every index is a compile-time constant after unrolling): bone b enters in front of the first
// slot it exceeds and pushes the rest down.
template <int K>
__global__ __launch_bounds__(kThreads) void skin_weights_kernel(
    const float* __restrict__ verts, int64_t V, const float* __restrict__ vol, int B, int G,
    const float* __restrict__ bbox_min, const float* __restrict__ bbox_scale, uint32_t* __restrict__ joints,
    float4* __restrict__ weights, float* __restrict__ kept_out) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const Trilinear t = trilinear_at(verts[3 * v + 0], verts[3 * v + 1], verts[3 * v + 2], bbox_min, bbox_scale, G);
    const size_t chan = (size_t)G * G * G;
    float s[K];
    unsigned j[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { s[k] = 0.f; j[k] = 0u; }
    for (int b = 0; b < B; ++b) {
        float cw = trilinear_channel(t, vol + b * chan);
        unsigned cj = (unsigned)b;
        bool moved = false;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool ins = moved || cw > s[k];
            const float ts = s[k];
            const unsigned tj = j[k];
            s[k] = ins ? cw : ts;
            j[k] = ins ? cj : tj;
            cw = ins ? ts : cw;
            cj = ins ? tj : cj;
            moved = ins;
        }
    }
    float kept = s[0];
#pragma unroll
    for (int k = 1; k < K; ++k) kept = kept + s[k];
    const bool ok = kept > 0.f;
    float w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        w[k] = ok ? s[k] / kept : (k == 0 ? 1.f : 0.f);
        j[k] = ok ? j[k] : 0u;
    }
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
        joints[v * (K / 4) + q] = j[4 * q] | (j[4 * q + 1] << 8) | (j[4 * q + 2] << 16) | (j[4 * q + 3] << 24);
        weights[v * (K / 4) + q] = make_float4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    }
    if (kept_out) kept_out[v] = kept;
}

template <int K>
__global__ __launch_bounds__(kThreads) void skin_lbs_kernel(const float* __restrict__ verts, int64_t V,
                                                            const uint32_t* __restrict__ joints,
                                                            const float4* __restrict__ weights,
                                                            const float* __restrict__ mats, int B,
                                                            float* __restrict__ out) {
    __shared__ float mat[kMaxSkinBones * 12];          // per bone: 3 x 4 row-major
    for (int i = threadIdx.x; i < 12 * B; i += kThreads) mat[i] = mats[i];
    __syncthreads();
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    const float x = verts[3 * v + 0], y = verts[3 * v + 1], z = verts[3 * v + 2];
    float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
        const uint32_t jw = joints[v * (K / 4) + q];
        const float4 w4 = weights[v * (K / 4) + q];
        const float wk[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int jb = (int)((jw >> (8 * e)) & 0xffu);
            if (jb >= B) continue;                     // (also keeps the read inside mat[])
            const float* m = mat + 12 * jb;
            const float px = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
            const float py = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
            const float pz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
            ax = ax + wk[e] * px;
            ay = ay + wk[e] * py;
            az = az + wk[e] * pz;
        }
    }
    out[3 * v + 0] = ax;
    out[3 * v + 1] = ay;
    out[3 * v + 2] = az;
}

}  // namespace
}  // namespace hnrf

using namespace hnrf;

extern "C" int hnrf_skin_weights(const float* verts, int64_t V, const float* vol, int B, int G, const float* bbox_min,
                                 const float* bbox_scale, int K, uint8_t* joints, float* weights, float* kept,
                                 void* stream) {
    HNRF_REQUIRE(V >= 0 && (V + kThreads - 1) / kThreads < 2147483647LL, HNRF_E_ARG, "hnrf_skin_weights: bad V=%lld",
                 (long long)V);
    HNRF_REQUIRE(K == 4 || K == 8, HNRF_E_ARG, "hnrf_skin_weights: K=%d, must be 4 or 8", K);
    HNRF_REQUIRE(B >= 1 && B <= kMaxSkinBones && G >= 2 && G <= 1024, HNRF_E_ARG,
                 "hnrf_skin_weights: bad dims B=%d G=%d (B <= %d)", B, G, kMaxSkinBones);
    if (V == 0) return HNRF_OK;
    HNRF_REQUIRE(verts && vol && bbox_min && bbox_scale && joints && weights, HNRF_E_ARG,
                 "hnrf_skin_weights: null pointer");
    HNRF_REQUIRE(((uintptr_t)joints & 3) == 0 && ((uintptr_t)weights & 15) == 0, HNRF_E_ARG,
                 "hnrf_skin_weights: joints must be 4-byte and weights 16-byte aligned");
    const dim3 grid((unsigned)((V + kThreads - 1) / kThreads));
    if (K == 4)
        hipLaunchKernelGGL(skin_weights_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, verts, V, vol, B, G,
                           bbox_min, bbox_scale, (uint32_t*)joints, (float4*)weights, kept);
    else
        hipLaunchKernelGGL(skin_weights_kernel<8>, grid, dim3(kThreads), 0, (hipStream_t)stream, verts, V, vol, B, G,
                           bbox_min, bbox_scale, (uint32_t*)joints, (float4*)weights, kept);
    return check_launch("hnrf_skin_weights");
}

extern "C" int hnrf_skin_lbs(const float* verts, int64_t V, const uint8_t* joints, const float* weights, int K,
                             const float* mats, int B, float* out, void* stream) {
    HNRF_REQUIRE(V >= 0 && (V + kThreads - 1) / kThreads < 2147483647LL, HNRF_E_ARG, "hnrf_skin_lbs: bad V=%lld",
                 (long long)V);
    HNRF_REQUIRE(K == 4 || K == 8, HNRF_E_ARG, "hnrf_skin_lbs: K=%d, must be 4 or 8", K);
    HNRF_REQUIRE(B >= 1 && B <= kMaxSkinBones, HNRF_E_ARG, "hnrf_skin_lbs: bad B=%d (1 <= B <= %d)", B, kMaxSkinBones);
    if (V == 0) return HNRF_OK;
    HNRF_REQUIRE(verts && joints && weights && mats && out, HNRF_E_ARG, "hnrf_skin_lbs: null pointer");
    HNRF_REQUIRE(((uintptr_t)joints & 3) == 0 && ((uintptr_t)weights & 15) == 0, HNRF_E_ARG,
                 "hnrf_skin_lbs: joints must be 4-byte and weights 16-byte aligned");
    const dim3 grid((unsigned)((V + kThreads - 1) / kThreads));
    if (K == 4)
        hipLaunchKernelGGL(skin_lbs_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, verts, V,
                           (const uint32_t*)joints, (const float4*)weights, mats, B, out);
    else
        hipLaunchKernelGGL(skin_lbs_kernel<8>, grid, dim3(kThreads), 0, (hipStream_t)stream, verts, V,
                           (const uint32_t*)joints, (const float4*)weights, mats, B, out);
    return check_launch("hnrf_skin_lbs");
}
