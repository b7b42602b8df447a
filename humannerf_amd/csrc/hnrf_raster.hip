// Rasteriser for vertex-coloured triangle meshes (the preview of the posed avatar mesh): a visibility buffer.
//
// Conventions: the module docstring of humannerf_amd/raster.py, which restates every kernel here in numpy bit for bit
// (this file is compiled with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt; float64 division is IEEE as
// the compiler emits it).  Four passes on one stream, nothing waits for the host:
//   clear       keys[H W] = 0, the count of the large list = 0, flip = det(K R) < 0 (one lane)
//   setup       one lane per vertex: project, snap to the 1/256-pixel grid, w = 1 / z -> 16-byte records
//   visibility  small instance: one lane per triangle; drop / cull, clamp the sample bbox to the image; a bbox of at
//               most kSmallSamples samples is walked by the lane, a larger one is appended to the large list (ballot +
//               popcount, one returning atomicAdd per wavefront); large instance: one wavefront per listed triangle
//               and per band of its bbox (up to kLargeSplit bands of at least kBandSamples samples, so that a triangle
//               that fills the screen is shared by 64 wavefronts), the lanes striding over the band (64 neighbouring
//               pixels = 512 contiguous bytes of keys per step).
//               An owned sample folds key = bits(w) << 32 | 0xFFFFFFFF - triangle into keys[pixel] with atomicMax
//               (a vector memory atomic on unsigned long long, no value returned: the lane does not wait for it).  The
//               maximum does not depend on the order of the folds: the outputs are bit-reproducible.  Reading the
//               pixel's key first and skipping an atomic that cannot win (-DHNRF_RASTER_EARLY_OUT) removes 20-47 % of the
//               atomics on the body meshes and makes the whole rasteriser up to 1.47x slower: a lane waits for every load
//               ("Mesh preview").
//   resolve     one lane per pixel: decode the key, recompute the winner's edge values, write rgb / alpha / depth /
//               tri_id.
#include <math.h>

#include "hnrf_common.h"

namespace hnrf {
namespace {

constexpr int kThreads = 256;
constexpr int kSmallSamples = 64;               // a sample bbox up to this size stays on the triangle's own lane
constexpr int kLargeBlocks = 4096;              // grid of the large instance (4 wavefronts each, striding the list)
constexpr unsigned kLargeSplit = 64;            // a listed triangle's bbox is cut into at most this many bands ...
constexpr unsigned kBandSamples = 16384;        // ... of at least this many samples, one wavefront each
constexpr float kGuardBand = 16384.0f;

struct alignas(16) RasterVertex {
    int X, Y;                                   // snapped screen position in 1/256 pixel
    float w;                                    // 1 / z; 0 = the vertex drops its triangles
    int pad;
};

struct RasterHeader {
    unsigned large_count;
    int flip;                                   // det(K R) < 0
    unsigned long long owned, atomics;          // -DHNRF_RASTER_COUNT (diagnostic build): samples owned / atomics issued
};

// Diagnostic builds (profiles/tools/time_mesh_render.py, through HNRF_LIB_PATH): -DHNRF_RASTER_COUNT counts the owned
// samples and the atomics issued into the header, -DHNRF_RASTER_EARLY_OUT skips the atomics that cannot win.
struct FoldCount {
    unsigned owned = 0, atomics = 0;
};

__device__ __forceinline__ void flush_count(const FoldCount& n, RasterHeader* head) {
#ifdef HNRF_RASTER_COUNT
    if (n.owned) atomicAdd(&head->owned, (unsigned long long)n.owned);
    if (n.atomics) atomicAdd(&head->atomics, (unsigned long long)n.atomics);
#endif
}

// workspace carve: vtx[V] | keys[H W] u64 | large[F] {triangle, bbox samples} | header
struct RasterCarve {
    RasterVertex* vtx;
    unsigned long long* keys;
    int2* large;
    RasterHeader* head;
    size_t bytes;
};

RasterCarve carve_raster(void* base, int64_t V, int64_t F, int H, int W) {
    size_t o = 0;
    auto take = [&](size_t n) {
        void* p = (void*)((uintptr_t)base + o);
        o += align256(n);
        return p;
    };
    RasterCarve c;
    c.vtx = (RasterVertex*)take((size_t)V * sizeof(RasterVertex));
    c.keys = (unsigned long long*)take((size_t)H * (size_t)W * 8);
    c.large = (int2*)take((size_t)F * 8);
    c.head = (RasterHeader*)take(sizeof(RasterHeader));
    c.bytes = o;
    return c;
}

__global__ __launch_bounds__(kThreads) void raster_clear_kernel(unsigned long long* __restrict__ keys, int64_t n,
                                                                const float* __restrict__ K, const float* __restrict__ R,
                                                                RasterHeader* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) keys[i] = 0ull;
    if (i == 0) {
        float M[3][3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) M[a][b] = (K[3 * a + 0] * R[b] + K[3 * a + 1] * R[3 + b]) + K[3 * a + 2] * R[6 + b];
        const float det = (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) -
                           M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])) +
                          M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
        head->large_count = 0u;
        head->owned = head->atomics = 0ull;
        head->flip = det < 0.f ? 1 : 0;
    }
}

__global__ __launch_bounds__(kThreads) void raster_setup_kernel(const float* __restrict__ verts, int64_t V,
                                                                const float* __restrict__ K, const float* __restrict__ R,
                                                                const float* __restrict__ T, float z_near,
                                                                RasterVertex* __restrict__ vtx) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= V) return;
    const float x = verts[3 * i + 0], y = verts[3 * i + 1], z = verts[3 * i + 2];
    float xc[3], p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) xc[a] = ((R[3 * a + 0] * x + R[3 * a + 1] * y) + R[3 * a + 2] * z) + T[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = (K[3 * a + 0] * xc[0] + K[3 * a + 1] * xc[1]) + K[3 * a + 2] * xc[2];
    const float u = p[0] / p[2], v = p[1] / p[2], w = 1.0f / xc[2];
    const bool ok = xc[2] >= z_near && fabsf(u) <= kGuardBand && fabsf(v) <= kGuardBand && w > 0.f;
    RasterVertex o;
    o.X = ok ? (int)rintf(256.0f * u) : 0;
    o.Y = ok ? (int)rintf(256.0f * v) : 0;
    o.w = ok ? w : 0.f;
    o.pad = 0;
    vtx[i] = o;
}

// A triangle that passed the drop and cull tests, in its own positive orientation (s = the sign of its area).
struct Tri {
    int64_t X[3], Y[3];
    int64_t s, A;                               // A = |area| > 0
    float w[3];
};

// Edge values E0, E1, E2 at the sample (sx, sy) in 1/256 pixel; they sum to A.
__device__ __forceinline__ void edge_values(const Tri& t, int64_t sx, int64_t sy, int64_t e[3]) {
    e[0] = t.s * ((t.X[2] - t.X[1]) * (sy - t.Y[1]) - (t.Y[2] - t.Y[1]) * (sx - t.X[1]));
    e[1] = t.s * ((t.X[0] - t.X[2]) * (sy - t.Y[2]) - (t.Y[0] - t.Y[2]) * (sx - t.X[2]));
    e[2] = t.s * ((t.X[1] - t.X[0]) * (sy - t.Y[0]) - (t.Y[1] - t.Y[0]) * (sx - t.X[0]));
}

// Loads triangle f; false when it is dropped (index out of range, dropped vertex, zero area).
__device__ __forceinline__ bool load_tri(const int* __restrict__ faces, int64_t f, int64_t V,
                                         const RasterVertex* __restrict__ vtx, Tri& t) {
    const int i0 = faces[3 * f + 0], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
    const RasterVertex a = vtx[i0], b = vtx[i1], c = vtx[i2];
    if (!(a.w > 0.f && b.w > 0.f && c.w > 0.f)) return false;
    t.X[0] = a.X; t.Y[0] = a.Y; t.w[0] = a.w;
    t.X[1] = b.X; t.Y[1] = b.Y; t.w[1] = b.w;
    t.X[2] = c.X; t.Y[2] = c.Y; t.w[2] = c.w;
    const int64_t area = (t.X[1] - t.X[0]) * (t.Y[2] - t.Y[0]) - (t.Y[1] - t.Y[0]) * (t.X[2] - t.X[0]);
    if (area == 0) return false;
    t.s = area < 0 ? -1 : 1;
    t.A = t.s * area;
    return true;
}

// Smallest edge value that owns the sample: 0 on a top or left edge of the oriented triangle, else 1.
__device__ __forceinline__ void tie_thresholds(const Tri& t, int64_t thr[3]) {
    const int from[3] = {1, 2, 0}, to[3] = {2, 0, 1};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t dx = t.s * (t.X[to[k]] - t.X[from[k]]), dy = t.s * (t.Y[to[k]] - t.Y[from[k]]);
        thr[k] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
    }
}

struct Box {
    int i0, j0, nx, ny;                         // clamped sample bbox; nx <= 0 or ny <= 0: empty
};

__device__ __forceinline__ Box sample_box(const Tri& t, int H, int W) {
    const int64_t xlo = min(min(t.X[0], t.X[1]), t.X[2]), xhi = max(max(t.X[0], t.X[1]), t.X[2]);
    const int64_t ylo = min(min(t.Y[0], t.Y[1]), t.Y[2]), yhi = max(max(t.Y[0], t.Y[1]), t.Y[2]);
    const int64_t i0 = max((xlo + 255) >> 8, (int64_t)0), i1 = min(xhi >> 8, (int64_t)W - 1);
    const int64_t j0 = max((ylo + 255) >> 8, (int64_t)0), j1 = min(yhi >> 8, (int64_t)H - 1);
    Box b;
    b.i0 = (int)i0; b.j0 = (int)j0;
    b.nx = (int)(i1 - i0 + 1); b.ny = (int)(j1 - j0 + 1);
    if (i1 < i0) b.nx = 0;
    if (j1 < j0) b.ny = 0;
    return b;
}

__device__ __forceinline__ float inv_depth(const Tri& t, const int64_t e[3]) {
    const double A = (double)t.A;
    const double b1 = (double)e[1] / A, b2 = (double)e[2] / A;
    const double w0 = (double)t.w[0], w1 = (double)t.w[1], w2 = (double)t.w[2];
    return (float)((w0 + b1 * (w1 - w0)) + b2 * (w2 - w0));
}

// Tests pixel (i, j) (inside the image) against the triangle and folds its key when the triangle owns the sample.
__device__ __forceinline__ void fold_sample(const Tri& t, const int64_t thr[3], unsigned tri, int i, int j, int W,
                                            unsigned long long* __restrict__ keys, FoldCount& n) {
    int64_t e[3];
    edge_values(t, (int64_t)i * 256, (int64_t)j * 256, e);
    if (e[0] < thr[0] || e[1] < thr[1] || e[2] < thr[2]) return;
    const float w = inv_depth(t, e);
    if (!(w > 0.f)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(w) << 32) | (unsigned long long)(0xFFFFFFFFu - tri);
    unsigned long long* cell = keys + (size_t)j * W + i;
    ++n.owned;
#ifdef HNRF_RASTER_EARLY_OUT
    if (*(volatile unsigned long long*)cell >= key) return;     // (keys only grow: a stale value is a smaller one)
#endif
    ++n.atomics;
    atomicMax(cell, key);
}

__global__ __launch_bounds__(kThreads) void raster_visibility_small_kernel(
    const int* __restrict__ faces, int64_t F, int64_t V, const RasterVertex* __restrict__ vtx, int H, int W, int cull,
    RasterHeader* __restrict__ head, int2* __restrict__ large, unsigned long long* __restrict__ keys) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    Tri t;
    Box b = {0, 0, 0, 0};
    bool live = f < F && load_tri(faces, f, V, vtx, t);
    if (live && cull != 0) {
        const bool front = (t.s < 0) != (head->flip != 0);
        live = (cull == HNRF_RASTER_CULL_BACK) ? front : !front;
    }
    if (live) {
        b = sample_box(t, H, W);
        live = b.nx > 0 && b.ny > 0;
    }
    const bool is_large = live && (int64_t)b.nx * b.ny > kSmallSamples;
    const unsigned long long ballot = __ballot(is_large);
    if (ballot) {                                                       // wave-uniform
        const int lane = threadIdx.x & (kWave - 1);
        const int leader = __ffsll((long long)ballot) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(&head->large_count, (unsigned)__popcll(ballot));
        base = __shfl(base, leader, kWave);
        if (is_large) large[base + __popcll(ballot & ((1ull << lane) - 1ull))] = make_int2((int)f, b.nx * b.ny);
    }
    if (!live || is_large) return;
    int64_t thr[3];
    tie_thresholds(t, thr);
    FoldCount n;
    for (int j = 0; j < b.ny; ++j)
        for (int i = 0; i < b.nx; ++i) fold_sample(t, thr, (unsigned)f, b.i0 + i, b.j0 + j, W, keys, n);
    flush_count(n, head);
}

__global__ __launch_bounds__(kThreads) void raster_visibility_large_kernel(
    const int* __restrict__ faces, int64_t V, const RasterVertex* __restrict__ vtx, int H, int W,
    RasterHeader* __restrict__ head, const int2* __restrict__ large, unsigned long long* __restrict__ keys) {
    const unsigned lane = threadIdx.x & (kWave - 1);
    const uint64_t waves = (uint64_t)gridDim.x * (kThreads / kWave);
    const unsigned count = head->large_count;
    const uint64_t items = (uint64_t)count * kLargeSplit;                // band-major: item = band * count + entry
    FoldCount cnt;
    for (uint64_t it = (uint64_t)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave; it < items; it += waves) {
        const unsigned band = (unsigned)(it / count);                   // wave-uniform from here on
        const int2 ent = large[it - (uint64_t)band * count];
        const unsigned n = (unsigned)ent.y;                             // <= 8192^2 = 2^26
        const unsigned bands = min(kLargeSplit, (n + kBandSamples - 1) / kBandSamples);
        if (band >= bands) continue;
        const unsigned chunk = ((n + bands - 1) / bands + (kWave - 1)) & ~(unsigned)(kWave - 1);
        const unsigned q0 = band * chunk, q1 = min(n, q0 + chunk);
        if (q0 >= q1) continue;
        const int f = ent.x;
        Tri t;
        if (!load_tri(faces, f, V, vtx, t)) continue;                   // (listed triangles passed this already)
        const Box b = sample_box(t, H, W);
        if (b.nx <= 0 || (unsigned)b.nx * (unsigned)b.ny != n) continue;
        int64_t thr[3];
        tie_thresholds(t, thr);
        for (unsigned q = q0 + lane; q < q1; q += kWave) {
            const unsigned j = q / (unsigned)b.nx, i = q - j * (unsigned)b.nx;
            fold_sample(t, thr, (unsigned)f, b.i0 + (int)i, b.j0 + (int)j, W, keys, cnt);
        }
    }
    flush_count(cnt, head);
}

__global__ __launch_bounds__(kThreads) void raster_resolve_kernel(
    const unsigned long long* __restrict__ keys, int H, int W, const float* __restrict__ verts,
    const int* __restrict__ faces, int64_t V, const float* __restrict__ colors, const RasterVertex* __restrict__ vtx,
    const float* __restrict__ R, const float* __restrict__ bgcolor, int shade_normal, float* __restrict__ rgb,
    float* __restrict__ alpha, float* __restrict__ depth, int* __restrict__ tri_id) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    const unsigned long long key = keys[p];
    if (key == 0ull) {
        if (rgb) { rgb[3 * p + 0] = bgcolor[0]; rgb[3 * p + 1] = bgcolor[1]; rgb[3 * p + 2] = bgcolor[2]; }
        if (alpha) alpha[p] = 0.f;
        if (depth) depth[p] = 0.f;
        if (tri_id) tri_id[p] = -1;
        return;
    }
    const unsigned f = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    const float w = __uint_as_float((unsigned)(key >> 32));
    if (alpha) alpha[p] = 1.f;
    if (depth) depth[p] = 1.0f / w;
    if (tri_id) tri_id[p] = (int)f;
    if (!rgb) return;
    const int i0 = faces[3 * (int64_t)f + 0], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
    float out[3];
    if (shade_normal) {
        const float* v0 = verts + 3 * (int64_t)i0;
        const float* v1 = verts + 3 * (int64_t)i1;
        const float* v2 = verts + 3 * (int64_t)i2;
        const float ax = v1[0] - v0[0], ay = v1[1] - v0[1], az = v1[2] - v0[2];
        const float bx = v2[0] - v0[0], by = v2[1] - v0[1], bz = v2[2] - v0[2];
        const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
        const bool good = len > 0.f && isfinite(len);
        const float mx = good ? cx / len : 0.f, my = good ? cy / len : 0.f, mz = good ? cz / len : 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a] = 0.5f + 0.5f * ((R[3 * a + 0] * mx + R[3 * a + 1] * my) + R[3 * a + 2] * mz);
    } else {
        Tri t;
        (void)load_tri(faces, f, V, vtx, t);                            // the winner passed it in the visibility pass
        int64_t e[3];
        const int j = (int)(p / W), i = (int)(p - (int64_t)j * W);
        edge_values(t, (int64_t)i * 256, (int64_t)j * 256, e);
        const double A = (double)t.A;
        const double q0 = (double)e[0] / A * (double)t.w[0], q1 = (double)e[1] / A * (double)t.w[1],
                     q2 = (double)e[2] / A * (double)t.w[2];
        const double den = (q0 + q1) + q2;
        const float* c0 = colors + 3 * (int64_t)i0;
        const float* c1 = colors + 3 * (int64_t)i1;
        const float* c2 = colors + 3 * (int64_t)i2;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            out[a] = (float)(((q0 * (double)c0[a] + q1 * (double)c1[a]) + q2 * (double)c2[a]) / den);
    }
    rgb[3 * p + 0] = out[0];
    rgb[3 * p + 1] = out[1];
    rgb[3 * p + 2] = out[2];
}

}  // namespace
}  // namespace hnrf

using namespace hnrf;

extern "C" size_t hnrf_raster_workspace_bytes(int64_t V, int64_t F, int H, int W) {
    if (V < 0 || V > 2147483647LL || F < 0 || F > 2147483647LL || H < 1 || H > 8192 || W < 1 || W > 8192) return 0;
    return carve_raster(nullptr, V, F, H, W).bytes;
}

extern "C" int hnrf_raster_mesh(const float* verts, int64_t V, const int* faces, int64_t F, const float* colors,
                                const float* K, const float* R, const float* T, const float* bgcolor, int H, int W,
                                float z_near, int flags, float* rgb, float* alpha, float* depth, int* tri_id,
                                void* workspace, size_t workspace_bytes, void* stream) {
    const bool shade_normal = (flags & HNRF_RASTER_SHADE_NORMAL) != 0;
    const int cull = flags & HNRF_RASTER_CULL_MASK;
    HNRF_REQUIRE(K && R && T && workspace, HNRF_E_ARG, "hnrf_raster_mesh: null pointer");
    HNRF_REQUIRE((V <= 0 || verts) && (F <= 0 || faces), HNRF_E_ARG, "hnrf_raster_mesh: null pointer (verts / faces)");
    HNRF_REQUIRE(!rgb || (bgcolor && (shade_normal || colors || V <= 0 || F <= 0)), HNRF_E_ARG,
                 "hnrf_raster_mesh: null pointer (rgb needs bgcolor, and colors unless the shade is normal)");
    HNRF_REQUIRE(H >= 1 && H <= 8192 && W >= 1 && W <= 8192, HNRF_E_UNSUPPORTED,
                 "hnrf_raster_mesh: image %dx%d out of range [1, 8192]", H, W);
    HNRF_REQUIRE(V >= 0 && V <= 2147483647LL && F >= 0 && F <= 2147483647LL, HNRF_E_UNSUPPORTED,
                 "hnrf_raster_mesh: bad counts V=%lld F=%lld (each < 2^31)", (long long)V, (long long)F);
    HNRF_REQUIRE(z_near > 0.f && isfinite(z_near), HNRF_E_UNSUPPORTED, "hnrf_raster_mesh: z_near must be positive and finite");
    HNRF_REQUIRE((flags & ~(HNRF_RASTER_CULL_MASK | HNRF_RASTER_SHADE_NORMAL)) == 0 && cull != 3, HNRF_E_UNSUPPORTED,
                 "hnrf_raster_mesh: unknown flags 0x%x", flags);
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0, HNRF_E_ARG, "hnrf_raster_mesh: workspace must be 256-byte aligned");
    const size_t need = hnrf_raster_workspace_bytes(V, F, H, W);
    HNRF_REQUIRE(workspace_bytes >= need, HNRF_E_WORKSPACE, "hnrf_raster_mesh: workspace %zu < %zu bytes", workspace_bytes, need);
    const RasterCarve c = carve_raster(workspace, V, F, H, W);
    hipStream_t st = (hipStream_t)stream;
    const int64_t npix = (int64_t)H * W;
    const unsigned pix_blocks = (unsigned)((npix + kThreads - 1) / kThreads);
    int rc;
    hipLaunchKernelGGL(raster_clear_kernel, dim3(pix_blocks), dim3(kThreads), 0, st, c.keys, npix, K, R, c.head);
    if ((rc = check_launch("hnrf_raster_mesh"))) return rc;
    if (V > 0 && F > 0) {
        hipLaunchKernelGGL(raster_setup_kernel, dim3((unsigned)((V + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, verts,
                           V, K, R, T, z_near, c.vtx);
        if ((rc = check_launch("hnrf_raster_mesh"))) return rc;
        const int64_t tri_blocks = (F + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(raster_visibility_small_kernel, dim3((unsigned)tri_blocks), dim3(kThreads), 0, st, faces, F, V,
                           c.vtx, H, W, cull, c.head, c.large, c.keys);
        if ((rc = check_launch("hnrf_raster_mesh"))) return rc;
        const int64_t wave_blocks = (F * kLargeSplit + kThreads / kWave - 1) / (kThreads / kWave);
        hipLaunchKernelGGL(raster_visibility_large_kernel, dim3((unsigned)(wave_blocks < kLargeBlocks ? wave_blocks : kLargeBlocks)),
                           dim3(kThreads), 0, st, faces, V, c.vtx, H, W, c.head, c.large, c.keys);
        if ((rc = check_launch("hnrf_raster_mesh"))) return rc;
    }
    if (rgb || alpha || depth || tri_id) {
        hipLaunchKernelGGL(raster_resolve_kernel, dim3(pix_blocks), dim3(kThreads), 0, st, c.keys, H, W, verts, faces, V,
                           colors, c.vtx, R, bgcolor, shade_normal ? 1 : 0, rgb, alpha, depth, tri_id);
        if ((rc = check_launch("hnrf_raster_mesh"))) return rc;
    }
    return HNRF_OK;
}
