// Surface records split by body part (hnrf_segment.h; humannerf_amd/cloud.py twin_segment / twin_compact is the numpy
// form, bit for bit).  Restates tools/segment.py:23-49 of the reference on the pixel grid: where the tool builds the
// (N, M, 2) tensor of pixel differences between all records and a part's seeds, a record here looks up the
// 2 r^2 - 2 r + 1 pixels of its L1 diamond in a per-frame bitmap of part masks -- rows and columns are integers, so the
// two select the same records.
//
//   segment_check_kernel    one lane per record: row, column and bone integer-valued, the pixel inside the image; the
//                           findings are ORed into the status word, which every later kernel reads first and, when it
//                           is not 0, returns without writing.
//   segment_seed_kernel     one lane per record ORs its bone's part mask into its pixel of its frame's bitmap
//                           (atomicOr: records may share a pixel; an OR does not depend on the order).
//   segment_gather_kernel   one lane per record ORs the bitmap words of its diamond, clipped to the image.  Records
//                           come in ray order, so a wave's lanes read neighbouring words of a row; a frame's bitmap
//                           (1 MB at 512 x 512) stays in L2.
//   segment_count_kernel    blocks of 256 packed rows: per part the number of kept rows (wave ballots).
//   segment_scan_kernel     one block: the exclusive scan over [part][block] (block_exclusive_scan, 64-bit carry).
//   segment_offsets_kernel  one lane per (part, frame): the base of the block the frame starts in + the kept rows of
//                           that block before the frame's first.
//   segment_scatter_kernel  a kept row's slot = its block's base + its rank in the block (wave totals + ballot).
// Within a part the kept rows of the packed array stay in order, and the frames lie in order: one stable compaction per
// part is the stable compaction per (part, frame).  No floating-point arithmetic beyond comparisons.
#include "hnrf_block_scan.h"

namespace hnrf {

constexpr int kSegMaxParts = 32, kSegMaxRadius = 64, kSegMaxSide = 16384;
constexpr int64_t kSegMaxWords = (int64_t)1 << 31;       // bitmap words of one batch (8 GiB)
constexpr int64_t kSegMaxTotal = ((int64_t)1 << 31) - 512;
enum { kSegBadPixel = 1, kSegOutside = 2, kSegBadBone = 4 };

// The frame of packed row n: the f with offsets[f] <= n < offsets[f + 1], -1 where there is none.  Whatever offsets
// hold, the result lies in [-1, F).
__device__ __forceinline__ int seg_frame(const int64_t* __restrict__ offsets, int F, int64_t n) {
    int lo = 0, hi = F;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid + 1] <= n) lo = mid + 1; else hi = mid;
    }
    return (lo < F && offsets[lo] <= n) ? lo : -1;
}

__device__ __forceinline__ bool seg_integer(float v) { return v == floorf(v) && fabsf(v) <= 16777216.f; }   // (NaN: false)

struct SegPixel {
    int r, c, bone, bad;      // bad: the status bits of this record; r, c, bone meaningful where it is 0
};
__device__ __forceinline__ SegPixel seg_pixel(const float* __restrict__ rec, int64_t n, int H, int W) {
    const float fr = rec[n * 10 + 7], fc = rec[n * 10 + 8], fb = rec[n * 10 + 9];
    SegPixel p{0, 0, 0, 0};
    if (!seg_integer(fr) || !seg_integer(fc)) p.bad |= kSegBadPixel;
    else {
        p.r = (int)fr;
        p.c = (int)fc;
        if (p.r < 0 || p.r >= H || p.c < 0 || p.c >= W) p.bad |= kSegOutside;
    }
    if (!seg_integer(fb)) p.bad |= kSegBadBone; else p.bone = (int)fb;
    return p;
}

__global__ __launch_bounds__(256) void segment_check_kernel(const float* __restrict__ rec, const int64_t* __restrict__ offsets,
                                                            int F, int64_t total, int H, int W, int* __restrict__ status) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int bad = 0;
    if (n < total && seg_frame(offsets, F, n) >= 0) bad = seg_pixel(rec, n, H, W).bad;
    if (__ballot(bad != 0) == 0) return;                                 // wave-uniform: the usual case
    if (bad) atomicOr(status, bad);
}

__global__ __launch_bounds__(256) void segment_seed_kernel(const float* __restrict__ rec, const int64_t* __restrict__ offsets,
                                                           int F, int64_t total, const uint32_t* __restrict__ bone_masks,
                                                           int B, int H, int W, uint32_t* __restrict__ seed,
                                                           const int* __restrict__ status) {
    if (*status != 0) return;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= total) return;
    const int f = seg_frame(offsets, F, n);
    if (f < 0) return;
    const SegPixel p = seg_pixel(rec, n, H, W);
    if (p.bad || p.bone < 0 || p.bone >= B) return;
    const uint32_t mask = bone_masks[p.bone];
    if (mask) atomicOr(seed + ((int64_t)f * H + p.r) * W + p.c, mask);
}

__global__ __launch_bounds__(256) void segment_gather_kernel(const float* __restrict__ rec, const int64_t* __restrict__ offsets,
                                                             int F, int64_t total, int H, int W, int radius,
                                                             const uint32_t* __restrict__ seed, uint32_t* __restrict__ member,
                                                             const int* __restrict__ status) {
    if (*status != 0) return;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= total) return;
    const int f = seg_frame(offsets, F, n);
    uint32_t m = 0;
    if (f >= 0) {
        const SegPixel p = seg_pixel(rec, n, H, W);
        if (!p.bad) {
            const uint32_t* bm = seed + (int64_t)f * H * W;
            for (int dr = 1 - radius; dr < radius; ++dr) {
                const int rr = p.r + dr;
                if (rr < 0 || rr >= H) continue;
                const int w = radius - 1 - (dr < 0 ? -dr : dr);
                const int c0 = p.c - w < 0 ? 0 : p.c - w, c1 = p.c + w > W - 1 ? W - 1 : p.c + w;
                const uint32_t* row = bm + (int64_t)rr * W;
                for (int cc = c0; cc <= c1; ++cc) m |= row[cc];
            }
        }
    }
    member[n] = m;
}

// ---- compaction
__device__ __forceinline__ uint32_t seg_kept(const uint32_t* __restrict__ member, const float* __restrict__ wrec, float wmin,
                                             int64_t n, int64_t total) {
    if (n >= total) return 0u;
    const uint32_t m = member[n];
    return (m && wrec && !(wrec[n * 10 + 6] > wmin)) ? 0u : m;
}

// cnt [P][nblk]
__global__ __launch_bounds__(256) void segment_count_kernel(const uint32_t* __restrict__ member, const float* __restrict__ wrec,
                                                            float wmin, int64_t total, int P, int64_t nblk,
                                                            const int* __restrict__ status, int* __restrict__ cnt) {
    __shared__ int wcnt[kScanThreads / kWave][kSegMaxParts];
    if (status && *status != 0) return;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t m = seg_kept(member, wrec, wmin, (int64_t)blockIdx.x * 256 + threadIdx.x, total);
    for (int p = 0; p < P; ++p) {
        const unsigned long long bal = __ballot((m >> p) & 1u);
        if (lane == 0) wcnt[wave][p] = __popcll(bal);
    }
    __syncthreads();
    if ((int)threadIdx.x < P) {
        const int p = threadIdx.x;
        cnt[p * nblk + blockIdx.x] = wcnt[0][p] + wcnt[1][p] + wcnt[2][p] + wcnt[3][p];
    }
}

// base [n + 1] = the exclusive scan of cnt [n], base[n] = the sum
__global__ __launch_bounds__(256) void segment_scan_kernel(const int* __restrict__ cnt, int64_t n, const int* __restrict__ status,
                                                           int64_t* __restrict__ base) {
    if (status && *status != 0) return;
    int64_t carry = 0;
    for (int64_t i0 = 0; i0 < n; i0 += kScanThreads) {                   // block-uniform
        const int64_t i = i0 + threadIdx.x;
        int tot;
        const int ex = block_exclusive_scan(i < n ? cnt[i] : 0, &tot);
        if (i < n) base[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) base[n] = carry;
}

__global__ __launch_bounds__(256) void segment_offsets_kernel(const uint32_t* __restrict__ member, const float* __restrict__ wrec,
                                                              float wmin, const int64_t* __restrict__ offsets, int F,
                                                              int64_t total, int P, int64_t nblk, const int* __restrict__ status,
                                                              const int64_t* __restrict__ base, int64_t* __restrict__ seg_offsets) {
    if (status && *status != 0) return;
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x, S = (int64_t)P * F;
    if (s > S) return;
    if (s == S) {
        seg_offsets[s] = base[P * nblk];
        return;
    }
    const int p = (int)(s / F), f = (int)(s % F);
    int64_t o = offsets[f];
    o = o < 0 ? 0 : o > total ? total : o;
    const int64_t b = o >> 8;                                            // (b = nblk: the next part's first base)
    int64_t acc = base[p * nblk + b];
    for (int64_t n = b << 8; n < o; ++n) acc += (seg_kept(member, wrec, wmin, n, total) >> p) & 1u;
    seg_offsets[s] = acc;
}

__global__ __launch_bounds__(256) void segment_scatter_kernel(const uint32_t* __restrict__ member, const float* __restrict__ wrec,
                                                              float wmin, int64_t total, int P, int64_t nblk,
                                                              const int* __restrict__ status, const int64_t* __restrict__ base,
                                                              int* __restrict__ src, int64_t src_rows) {
    __shared__ int wcnt[kScanThreads / kWave][kSegMaxParts];
    if (status && *status != 0) return;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t m = seg_kept(member, wrec, wmin, n, total);
    for (int p = 0; p < P; ++p) {
        const unsigned long long bal = __ballot((m >> p) & 1u);
        if (lane == 0) wcnt[wave][p] = __popcll(bal);
    }
    __syncthreads();
    for (int p = 0; p < P; ++p) {
        const unsigned long long bal = __ballot((m >> p) & 1u);
        if ((m >> p) & 1u) {
            int rank = __popcll(bal & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) rank += wcnt[w][p];
            const int64_t pos = base[p * nblk + blockIdx.x] + rank;
            if (pos >= 0 && pos < src_rows) src[pos] = (int)n;
        }
    }
}

static inline int64_t seg_blocks(int64_t total) { return (total + 255) / 256; }
static inline bool seg_compact_sizes_ok(int64_t total, int P) {
    return total >= 0 && total <= kSegMaxTotal && P >= 1 && P <= kSegMaxParts;
}

}  // namespace hnrf

using namespace hnrf;

extern "C" size_t hnrf_segment_workspace_bytes(int n_frames, int H, int W) {
    if (n_frames < 0 || H < 1 || W < 1 || H > kSegMaxSide || W > kSegMaxSide) return 0;
    const int64_t words = (int64_t)n_frames * H * W;
    if (words > kSegMaxWords) return 0;
    return align256((size_t)(words > 0 ? words : 1) * sizeof(uint32_t));
}

extern "C" int hnrf_segment_members(const float* rec, const int64_t* offsets, int n_frames, int64_t total,
                                    const uint32_t* bone_masks, int n_bones, int H, int W, int radius, void* workspace,
                                    size_t workspace_bytes, uint32_t* member, int* status, void* stream) {
    HNRF_REQUIRE(radius >= 1 && radius <= kSegMaxRadius, HNRF_E_ARG, "hnrf_segment_members: radius %d (1 .. %d)", radius,
                 kSegMaxRadius);
    HNRF_REQUIRE(n_bones >= 1 && n_bones <= kSegMaxParts, HNRF_E_ARG, "hnrf_segment_members: n_bones %d (1 .. %d)", n_bones,
                 kSegMaxParts);
    HNRF_REQUIRE(H >= 1 && H <= kSegMaxSide, HNRF_E_ARG, "hnrf_segment_members: H %d (1 .. %d)", H, kSegMaxSide);
    HNRF_REQUIRE(W >= 1 && W <= kSegMaxSide, HNRF_E_ARG, "hnrf_segment_members: W %d (1 .. %d)", W, kSegMaxSide);
    HNRF_REQUIRE(n_frames >= 0, HNRF_E_ARG, "hnrf_segment_members: n_frames %d", n_frames);
    HNRF_REQUIRE(total >= 0 && total <= kSegMaxTotal, HNRF_E_ARG, "hnrf_segment_members: total %lld", (long long)total);
    const size_t need = hnrf_segment_workspace_bytes(n_frames, H, W);
    HNRF_REQUIRE(need != 0, HNRF_E_UNSUPPORTED, "hnrf_segment_members: n_frames %d of %d x %d pixels exceed one batch (2^31)",
                 n_frames, H, W);
    HNRF_REQUIRE(status && offsets && bone_masks && workspace && (total == 0 || (rec && member)), HNRF_E_ARG,
                 "hnrf_segment_members: null pointer");
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)offsets & 7) == 0, HNRF_E_ARG,
                 "hnrf_segment_members: workspace must be 256-byte aligned, offsets 8-byte aligned");
    HNRF_REQUIRE(workspace_bytes >= need, HNRF_E_WORKSPACE, "hnrf_segment_members: workspace of %zu bytes, %zu needed",
                 workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess ||
        (total > 0 && n_frames > 0 && hipMemsetAsync(workspace, 0, need, st) != hipSuccess)) {
        set_error("hnrf_segment_members: hipMemsetAsync failed");
        return HNRF_E_LAUNCH;
    }
    if (total == 0) return HNRF_OK;
    const dim3 grid((unsigned)seg_blocks(total)), block(256);
    uint32_t* seed = (uint32_t*)workspace;
    hipLaunchKernelGGL(segment_check_kernel, grid, block, 0, st, rec, offsets, n_frames, total, H, W, status);
    hipLaunchKernelGGL(segment_seed_kernel, grid, block, 0, st, rec, offsets, n_frames, total, bone_masks, n_bones, H, W, seed,
                       (const int*)status);
    hipLaunchKernelGGL(segment_gather_kernel, grid, block, 0, st, rec, offsets, n_frames, total, H, W, radius,
                       (const uint32_t*)seed, member, (const int*)status);
    return check_launch("hnrf_segment_members");
}

extern "C" size_t hnrf_segment_compact_workspace_bytes(int64_t total, int n_parts) {
    if (!seg_compact_sizes_ok(total, n_parts)) return 0;
    const size_t n = (size_t)n_parts * (size_t)seg_blocks(total);
    return align256((n + 1) * sizeof(int64_t)) + align256((n ? n : 1) * sizeof(int));
}

extern "C" int hnrf_segment_count(const uint32_t* member, const float* weight_rec, float weight_min, const int64_t* offsets,
                                  int n_frames, int64_t total, int n_parts, const int* status, void* workspace,
                                  size_t workspace_bytes, int64_t* seg_offsets, void* stream) {
    HNRF_REQUIRE(n_parts >= 1 && n_parts <= kSegMaxParts, HNRF_E_ARG, "hnrf_segment_count: n_parts %d (1 .. %d)", n_parts,
                 kSegMaxParts);
    HNRF_REQUIRE(n_frames >= 0 && n_frames <= (1 << 24), HNRF_E_ARG, "hnrf_segment_count: n_frames %d", n_frames);
    HNRF_REQUIRE(total >= 0 && total <= kSegMaxTotal, HNRF_E_ARG, "hnrf_segment_count: total %lld", (long long)total);
    HNRF_REQUIRE(weight_min == weight_min, HNRF_E_ARG, "hnrf_segment_count: weight_min is NaN");
    HNRF_REQUIRE(offsets && seg_offsets && workspace && (total == 0 || member), HNRF_E_ARG, "hnrf_segment_count: null pointer");
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)offsets & 7) == 0 && ((uintptr_t)seg_offsets & 7) == 0,
                 HNRF_E_ARG, "hnrf_segment_count: workspace must be 256-byte aligned, offsets and seg_offsets 8-byte aligned");
    const size_t need = hnrf_segment_compact_workspace_bytes(total, n_parts);
    HNRF_REQUIRE(workspace_bytes >= need, HNRF_E_WORKSPACE, "hnrf_segment_count: workspace of %zu bytes, %zu needed",
                 workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nblk = seg_blocks(total), n = (int64_t)n_parts * nblk;
    int64_t* base = (int64_t*)workspace;
    int* cnt = (int*)((char*)workspace + align256((size_t)(n + 1) * sizeof(int64_t)));
    if (nblk > 0)
        hipLaunchKernelGGL(segment_count_kernel, dim3((unsigned)nblk), dim3(256), 0, st, member, weight_rec, weight_min, total,
                           n_parts, nblk, status, cnt);
    hipLaunchKernelGGL(segment_scan_kernel, dim3(1), dim3(256), 0, st, (const int*)cnt, n, status, base);
    const int64_t S = (int64_t)n_parts * n_frames + 1;
    hipLaunchKernelGGL(segment_offsets_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, member, weight_rec,
                       weight_min, offsets, n_frames, total, n_parts, nblk, status, (const int64_t*)base, seg_offsets);
    return check_launch("hnrf_segment_count");
}

extern "C" int hnrf_segment_scatter(const uint32_t* member, const float* weight_rec, float weight_min, int64_t total,
                                    int n_parts, const int* status, const void* workspace, size_t workspace_bytes, int* src,
                                    int64_t src_rows, void* stream) {
    HNRF_REQUIRE(n_parts >= 1 && n_parts <= kSegMaxParts, HNRF_E_ARG, "hnrf_segment_scatter: n_parts %d (1 .. %d)", n_parts,
                 kSegMaxParts);
    HNRF_REQUIRE(total >= 0 && total <= kSegMaxTotal, HNRF_E_ARG, "hnrf_segment_scatter: total %lld", (long long)total);
    HNRF_REQUIRE(src_rows >= 0, HNRF_E_ARG, "hnrf_segment_scatter: src_rows %lld", (long long)src_rows);
    HNRF_REQUIRE(weight_min == weight_min, HNRF_E_ARG, "hnrf_segment_scatter: weight_min is NaN");
    if (total == 0 || src_rows == 0) return HNRF_OK;
    HNRF_REQUIRE(member && workspace && src, HNRF_E_ARG, "hnrf_segment_scatter: null pointer");
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0, HNRF_E_ARG, "hnrf_segment_scatter: workspace must be 256-byte aligned");
    const size_t need = hnrf_segment_compact_workspace_bytes(total, n_parts);
    HNRF_REQUIRE(workspace_bytes >= need, HNRF_E_WORKSPACE, "hnrf_segment_scatter: workspace of %zu bytes, %zu needed",
                 workspace_bytes, need);
    const int64_t nblk = seg_blocks(total);
    hipLaunchKernelGGL(segment_scatter_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, member, weight_rec,
                       weight_min, total, n_parts, nblk, status, (const int64_t*)workspace, src, src_rows);
    return check_launch("hnrf_segment_scatter");
}
