// Surface-point records and the frame x frame appearance distance (hnrf_cloud.h; humannerf_amd/cloud.py is the host
// twin of everything here, bit for bit).  Restates run.py:391-396 (one canonical surface point per ray) and
// tools/compute_distance*.py (mutual nearest neighbours of two frames' point clouds closer than dist_thresh, summed
// colour error) of the reference.
//
// One arithmetic statement, compiled without contraction and with the correctly rounded sqrt (Makefile):
//   d2(a, b) = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)),  dx = fl(ax - bx)           (symmetric in a, b bit for bit)
//   the nearest neighbour = smallest d2, ties to the LOWEST ORIGINAL RECORD INDEX; a distance = fl(sqrt(d2));
//   the colour error = the same expression on the rgb columns.
//
//   surface_points_kernel  one wave per ray (4 per workgroup, as K4).  Lane l adds the samples l, l + 64, l + 128 ...
//                          in ascending order (acc = fl(acc + fl(w x))), then a 6-step xor butterfly (32, 16 .. 1)
//                          adds the lanes: the order depends on S alone, never on R or on the launch.
//   cloud_nn_kernel        brute force: one lane per point of a, cloud b staged through LDS in tiles of 1024 points
//                          and walked in index order with a strict <, so the lowest index of equal d2 wins.
//   cloud_pairs_kernel     one lane per point p of frame i of a pair (i, j); both frames sorted along one coordinate.
//                          The window of p is |k_p - k_q| <= tau (1 + 2^-20), bounds in fp64.  A workgroup's 256 points
//                          are neighbours along that coordinate: two binary searches bound the UNION of their windows,
//                          which goes through LDS in tiles exactly as in cloud_nn_kernel (broadcast reads), every lane
//                          taking the argmin of d2 (ties by orig) over it; if fl(sqrt(d2)) < tau the same search runs
//                          back from the winners q into frame i (the union of the q's windows), and where it returns p
//                          the pair adds its colour error.  The union decides as the lane's own window does.
//                          DESIGN.md section 4 "Surface points and frame distance" has the argument that the window
//                          holds every candidate that can win, so that the result is the brute-force one.
//   cloud_pairs_sum_kernel one lane per pair adds that pair's workgroup partials in block order.
// No atomics: every sum has one fixed order, two runs give the same bits.
#include "hnrf_common.h"

namespace hnrf {

constexpr int kCloudTile = 1024;        // points of cloud b per LDS tile (12 KiB)
constexpr int kPairGridY = 65535;       // pairs per launch (gridDim.y)

__device__ __forceinline__ float cloud_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// ---- surface points
__global__ __launch_bounds__(256) void surface_points_kernel(const float* __restrict__ weights, const float* __restrict__ xyz,
                                                             const float* __restrict__ bmw, int64_t R, int S, int B,
                                                             float* __restrict__ wxyz, float* __restrict__ wmax,
                                                             int* __restrict__ lbs) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= R) return;   // wave-uniform
    const int64_t base = ray * S;
    float sx = 0.f, sy = 0.f, sz = 0.f, mx = -__builtin_inff();
    float acc[32];
#pragma unroll
    for (int b = 0; b < 32; ++b) acc[b] = 0.f;
    for (int s = lane; s < S; s += 64) {
        const float w = weights[base + s];
        const float* p = xyz + (base + s) * 3;
        sx = sx + w * p[0];
        sy = sy + w * p[1];
        sz = sz + w * p[2];
        mx = fmaxf(mx, w);
        const float* q = bmw + (base + s) * B;
#pragma unroll
        for (int b = 0; b < 32; ++b)
            if (b < B) acc[b] = acc[b] + w * q[b];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sx = sx + __shfl_xor(sx, off, 64);
        sy = sy + __shfl_xor(sy, off, 64);
        sz = sz + __shfl_xor(sz, off, 64);
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    }
    float best = 0.f;
    int ibest = 0;
#pragma unroll
    for (int b = 0; b < 32; ++b) {
        if (b < B) {                                                     // wave-uniform
            float v = acc[b];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
            if (b == 0 || v > best) { best = v; ibest = b; }             // strict >: the lowest index of equal sums
        }
    }
    if (lane == 0) {
        wxyz[ray * 3 + 0] = sx;
        wxyz[ray * 3 + 1] = sy;
        wxyz[ray * 3 + 2] = sz;
        wmax[ray] = mx;
        lbs[ray] = ibest;
    }
}

// ---- brute-force nearest neighbour
__global__ __launch_bounds__(256) void cloud_nn_kernel(const float* __restrict__ a, int64_t Na, const float* __restrict__ b,
                                                       int64_t Nb, int* __restrict__ idx, float* __restrict__ d2) {
    __shared__ float tx[kCloudTile], ty[kCloudTile], tz[kCloudTile];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < Na;
    const float ax = in ? a[i * 3] : 0.f, ay = in ? a[i * 3 + 1] : 0.f, az = in ? a[i * 3 + 2] : 0.f;
    float best = __builtin_inff();
    int ibest = -1;
    for (int64_t t0 = 0; t0 < Nb; t0 += kCloudTile) {
        const int n = (int)(Nb - t0 < kCloudTile ? Nb - t0 : kCloudTile);
        for (int k = threadIdx.x; k < n; k += 256) {
            tx[k] = b[(t0 + k) * 3];
            ty[k] = b[(t0 + k) * 3 + 1];
            tz[k] = b[(t0 + k) * 3 + 2];
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {                                    // every lane reads the same word: a broadcast
            const float d = cloud_d2(ax, ay, az, tx[k], ty[k], tz[k]);
            if (d < best) { best = d; ibest = (int)(t0 + k); }
        }
        __syncthreads();
    }
    if (in) {
        idx[i] = ibest;
        d2[i] = best;
    }
}

// ---- windowed search in one sorted frame: points [0, n) at xyz / orig, keys = coordinate `axis`
struct CloudHit {
    int pos, orig;         // position in the sorted frame and original record index of the winner; pos -1 = none
    float d2;
};
// first position whose key is >= k (upper = false) or > k (upper = true), compared in fp64
__device__ __forceinline__ int cloud_bound(const float* __restrict__ xyz, int n, int axis, double k, bool upper) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double v = (double)xyz[(int64_t)mid * 3 + axis];
        if (upper ? v <= k : v < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// The workgroup's search: its points' keys lie in [kmin, kmax], so the union of their windows is the rows
// [first key >= kmin - win, first key > kmax + win) of the frame.  Those go through LDS in tiles and every lane that is
// `on` takes the argmin of d2 over ALL of them, ties by orig.  A superset of the lane's own window decides the same:
// what lies outside the window is farther than tau and cannot beat, or tie with, a minimum below tau -- and a minimum
// that is not below tau is dropped by the caller whichever candidate holds it.  Block-uniform control flow.
__device__ __forceinline__ CloudHit cloud_block_nn(const float* __restrict__ xyz, const int* __restrict__ orig, int n, int axis,
                                                   double win, float kmin, float kmax, bool on, float ax, float ay, float az,
                                                   float* tx, float* ty, float* tz, int* to) {
    const int first = cloud_bound(xyz, n, axis, (double)kmin - win, false);
    const int last = cloud_bound(xyz, n, axis, (double)kmax + win, true);
    CloudHit h{-1, 0x7fffffff, __builtin_inff()};
    for (int t0 = first; t0 < last; t0 += kCloudTile) {
        const int m = last - t0 < kCloudTile ? last - t0 : kCloudTile;
        for (int k = threadIdx.x; k < m; k += 256) {
            const float* q = xyz + (int64_t)(t0 + k) * 3;
            tx[k] = q[0]; ty[k] = q[1]; tz[k] = q[2];
            to[k] = orig[t0 + k];
        }
        __syncthreads();
        if (on) {
            for (int k = 0; k < m; ++k) {                                // every lane reads the same word: a broadcast
                const float d = cloud_d2(ax, ay, az, tx[k], ty[k], tz[k]);
                if (d <= h.d2) {
                    const int o = to[k];
                    if (d < h.d2 || o < h.orig) { h.pos = t0 + k; h.orig = o; h.d2 = d; }
                }
            }
        }
        __syncthreads();
    }
    return h;
}

// grid (blocks of frame i's points, pairs of this launch).  part [pairs][gridDim.x] fp64; match nullable [pairs][max_n].
__global__ __launch_bounds__(256) void cloud_pairs_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb,
                                                          const int* __restrict__ orig, const int64_t* __restrict__ offsets,
                                                          int F, int64_t total, const int* __restrict__ pairs, int64_t max_n,
                                                          int axis, float tau, double win, double* __restrict__ part,
                                                          int* __restrict__ match) {
    __shared__ float tx[kCloudTile], ty[kCloudTile], tz[kCloudTile];
    __shared__ int to[kCloudTile];
    __shared__ double red[256];
    __shared__ float kq[2][256];
    const int tid = threadIdx.x;
    const int64_t pr = blockIdx.y;
    const int fi = pairs[pr * 2], fj = pairs[pr * 2 + 1];
    int64_t oi = 0, oj = 0, ni = 0, nj = 0;
    if (fi >= 0 && fi < F && fj >= 0 && fj < F) {
        oi = offsets[fi]; ni = offsets[fi + 1] - oi;
        oj = offsets[fj]; nj = offsets[fj + 1] - oj;
        // a frame that does not lie inside the packed arrays counts as empty
        if (oi < 0 || ni < 0 || oi + ni > total || ni > max_n) ni = 0;
        if (oj < 0 || nj < 0 || oj + nj > total || nj > max_n) nj = 0;
    }
    const int64_t p0 = (int64_t)blockIdx.x * 256, p = p0 + tid;
    if (p0 >= ni) {                                                      // block-uniform: past frame i's count
        if (match && p < max_n) match[pr * max_n + p] = -1;
        return;
    }
    const float* xi = xyz + oi * 3;
    const float* xj = xyz + oj * 3;
    const bool in = p < ni;
    const int64_t pc = in ? p : ni - 1;
    const float ax = xi[pc * 3], ay = xi[pc * 3 + 1], az = xi[pc * 3 + 2];
    const int64_t pl = p0 + 255 < ni ? p0 + 255 : ni - 1;
    // 1, 2: the nearest neighbour in frame j (the frame is sorted: the block's keys run from its first to its last point)
    const CloudHit q = cloud_block_nn(xj, orig + oj, (int)nj, axis, win, xi[p0 * 3 + axis], xi[pl * 3 + axis], in, ax, ay, az,
                                      tx, ty, tz, to);
    // 3: from the winners closer than tau back into frame i; their keys span the staged range
    const bool near = in && q.pos >= 0 && sqrtf(q.d2) < tau;
    const int qc = near ? q.pos : 0;
    float bx = 0.f, by = 0.f, bz = 0.f;
    if (near) { bx = xj[(int64_t)qc * 3]; by = xj[(int64_t)qc * 3 + 1]; bz = xj[(int64_t)qc * 3 + 2]; }
    const float kb = axis == 0 ? bx : axis == 1 ? by : bz;
    kq[0][tid] = near ? kb : __builtin_inff();
    kq[1][tid] = near ? kb : -__builtin_inff();
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            kq[0][tid] = fminf(kq[0][tid], kq[0][tid + s]);
            kq[1][tid] = fmaxf(kq[1][tid], kq[1][tid + s]);
        }
        __syncthreads();
    }
    const float kqmin = kq[0][0], kqmax = kq[1][0];
    double err = 0.0;
    int partner = -1;
    if (kqmin <= kqmax) {                                                // block-uniform: some lane has a winner below tau
        const CloudHit back = cloud_block_nn(xi, orig + oi, (int)ni, axis, win, kqmin, kqmax, near, bx, by, bz, tx, ty, tz, to);
        if (near && back.pos == (int)p) {                                // 4
            const float* ca = rgb + (oi + p) * 3;
            const float* cb = rgb + (oj + q.pos) * 3;
            err = (double)sqrtf(cloud_d2(ca[0], ca[1], ca[2], cb[0], cb[1], cb[2]));
            partner = q.orig;
        }
    }
    if (match && p < max_n) match[pr * max_n + p] = partner;
    // the workgroup's sum in thread order: lane 16 g adds the lanes 16 g .. 16 g + 15 ascending, lane 0 the 16 groups
    red[tid] = err;
    __syncthreads();
    if ((tid & 15) == 0) {
        double s = red[tid];
        for (int k = 1; k < 16; ++k) s = s + red[tid + k];
        red[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double s = red[0];
        for (int k = 16; k < 256; k += 16) s = s + red[k];
        part[pr * gridDim.x + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void cloud_pairs_sum_kernel(const int64_t* __restrict__ offsets, int F, int64_t total,
                                                              const int* __restrict__ pairs, int n_pairs, int64_t max_n,
                                                              int nblk, const double* __restrict__ part,
                                                              double* __restrict__ D) {
    const int pr = blockIdx.x * 256 + threadIdx.x;
    if (pr >= n_pairs) return;
    const int fi = pairs[pr * 2], fj = pairs[pr * 2 + 1];
    int64_t ni = 0;
    if (fi >= 0 && fi < F && fj >= 0 && fj < F) {
        const int64_t oi = offsets[fi];
        ni = offsets[fi + 1] - oi;
        if (oi < 0 || ni < 0 || oi + ni > total || ni > max_n) ni = 0;
    }
    int64_t nb = (ni + 255) / 256;                                       // the blocks that wrote a partial
    if (nb > nblk) nb = nblk;
    double s = 0.0;
    for (int64_t k = 0; k < nb; ++k) s = s + part[(int64_t)pr * nblk + k];
    D[pr] = s;
}

static inline bool pairs_sizes_ok(int64_t n_pairs, int64_t max_n) {
    return n_pairs >= 0 && n_pairs <= ((int64_t)1 << 40) && max_n >= 0 && max_n <= ((int64_t)1 << 24);
}

}  // namespace hnrf

using namespace hnrf;

extern "C" int hnrf_surface_points(const float* weights, const float* xyz, const float* bmw, int64_t R, int S, int B,
                                   float* wxyz, float* wmax, int* lbs, void* stream) {
    HNRF_REQUIRE(R >= 0 && S >= 1 && B >= 1, HNRF_E_ARG, "hnrf_surface_points: bad dims R=%lld S=%d B=%d", (long long)R, S, B);
    HNRF_REQUIRE(S <= 512 && B <= 32, HNRF_E_UNSUPPORTED, "hnrf_surface_points: S=%d B=%d (S <= 512, B <= 32 built)", S, B);
    if (R == 0) return HNRF_OK;        // (no rays: the pointers are not looked at, as in hnrf_cloud_nn for Na = 0)
    HNRF_REQUIRE(weights && xyz && bmw && wxyz && wmax && lbs, HNRF_E_ARG, "hnrf_surface_points: null pointer");
    const int64_t blocks = (R + 3) / 4;
    HNRF_REQUIRE(blocks < (int64_t)2147483647, HNRF_E_ARG, "hnrf_surface_points: too many rays");
    hipLaunchKernelGGL(surface_points_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, weights, xyz, bmw, R,
                       S, B, wxyz, wmax, lbs);
    return check_launch("hnrf_surface_points");
}

extern "C" int hnrf_cloud_nn(const float* a, int64_t Na, const float* b, int64_t Nb, int* idx, float* d2, void* stream) {
    HNRF_REQUIRE(Na >= 0 && Nb >= 0, HNRF_E_ARG, "hnrf_cloud_nn: bad sizes Na=%lld Nb=%lld", (long long)Na, (long long)Nb);
    HNRF_REQUIRE(Na <= 0x7fffffff && Nb <= 0x7fffffff, HNRF_E_UNSUPPORTED, "hnrf_cloud_nn: more than 2^31 - 1 points");
    if (Na == 0) return HNRF_OK;
    HNRF_REQUIRE(a && idx && d2 && (b || Nb == 0), HNRF_E_ARG, "hnrf_cloud_nn: null pointer");
    hipLaunchKernelGGL(cloud_nn_kernel, dim3((unsigned)((Na + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, Na, b, Nb,
                       idx, d2);
    return check_launch("hnrf_cloud_nn");
}

extern "C" size_t hnrf_cloud_distance_pairs_workspace_bytes(int64_t n_pairs, int64_t max_n) {
    if (!pairs_sizes_ok(n_pairs, max_n)) return 0;
    const int64_t per = n_pairs < kPairGridY ? n_pairs : kPairGridY;     // one launch's partials; launches reuse them
    const int64_t nblk = (max_n + 255) / 256;
    return align256((size_t)(per * nblk > 0 ? per * nblk : 1) * sizeof(double));
}

extern "C" int hnrf_cloud_distance_pairs(const float* xyz, const float* rgb, const int* orig, const int64_t* offsets,
                                         int n_frames, int64_t total, const int* pairs, int64_t n_pairs, int64_t max_n,
                                         int axis, float tau, void* workspace, size_t workspace_bytes, double* D, int* match,
                                         void* stream) {
    HNRF_REQUIRE(tau > 0.f && tau <= 3.4028234663852886e38f, HNRF_E_ARG,
                 "hnrf_cloud_distance_pairs: tau %g must be finite and > 0", (double)tau);        // (NaN fails both)
    HNRF_REQUIRE(axis >= 0 && axis <= 2, HNRF_E_ARG, "hnrf_cloud_distance_pairs: axis %d", axis);
    HNRF_REQUIRE(n_frames >= 0 && total >= 0 && pairs_sizes_ok(n_pairs, max_n), HNRF_E_ARG,
                 "hnrf_cloud_distance_pairs: bad sizes F=%d total=%lld pairs=%lld max_n=%lld", n_frames, (long long)total,
                 (long long)n_pairs, (long long)max_n);
    if (n_pairs == 0) return HNRF_OK;
    HNRF_REQUIRE(offsets && pairs && D && workspace && (total == 0 || (xyz && rgb && orig)), HNRF_E_ARG,
                 "hnrf_cloud_distance_pairs: null pointer");
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)D & 7) == 0 && ((uintptr_t)offsets & 7) == 0, HNRF_E_ARG,
                 "hnrf_cloud_distance_pairs: workspace must be 256-byte aligned, D and offsets 8-byte aligned");
    const size_t need = hnrf_cloud_distance_pairs_workspace_bytes(n_pairs, max_n);
    HNRF_REQUIRE(workspace_bytes >= need, HNRF_E_WORKSPACE, "hnrf_cloud_distance_pairs: workspace of %zu bytes, %zu needed",
                 workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)((max_n + 255) / 256);
    const double win = (double)tau * (1.0 + 9.5367431640625e-07);        // tau (1 + 2^-20)
    double* part = (double*)workspace;
    for (int64_t p0 = 0; p0 < n_pairs; p0 += kPairGridY) {
        const int n = (int)(n_pairs - p0 < kPairGridY ? n_pairs - p0 : kPairGridY);
        if (nblk > 0)
            hipLaunchKernelGGL(cloud_pairs_kernel, dim3(nblk, n), dim3(256), 0, st, xyz, rgb, orig, offsets, n_frames, total,
                               pairs + p0 * 2, max_n, axis, tau, win, part, match ? match + p0 * max_n : nullptr);
        hipLaunchKernelGGL(cloud_pairs_sum_kernel, dim3((n + 255) / 256), dim3(256), 0, st, offsets, n_frames, total,
                           pairs + p0 * 2, n, max_n, nblk, part, D + p0);
    }
    return check_launch("hnrf_cloud_distance_pairs");
}
