// Block-level scans and stream compaction for 256-thread blocks (four waves of 64), and the one device statement of the
// shared-sample classification built on them.  A header: hnrf_mesh.o is compiled with flags of its own.
// Every thread of the block must reach a call (barriers inside).
#pragma once
#include "hnrf_common.h"

namespace hnrf {

constexpr int kScanThreads = 256;

// Number of threads before this one, in thread order, whose `keep` is set; *total = the block's count.  Ballot /
// popcount inside a wave, the four wave totals through LDS.  ONE CALL PER KERNEL, block_append's included: no barrier
// stands behind the last read of the totals, so a second call could overwrite them under a slower wave (a barrier here
// would be paid by every K1 block; no kernel needs two).
__device__ __forceinline__ int block_rank(bool keep, int* total) {
    __shared__ int wave_tot[kScanThreads / kWave];
    const unsigned long long bal = __ballot(keep);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += wave_tot[w];
    *total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    return before;
}

// Stream compaction: the slot of this thread's element in the list that *count counts (meaningful where `keep`).  The
// block takes its run with one atomicAdd by thread 0 -- block-contiguous runs, blocks in arrival order; an empty block
// issues no atomic.
__device__ __forceinline__ int block_append(bool keep, int* count) {
    __shared__ int block_base;
    int total;
    const int rank = block_rank(keep, &total);
    if (threadIdx.x == 0) block_base = total ? atomicAdd(count, total) : 0;
    __syncthreads();
    return block_base + rank;
}

// Exclusive prefix of v over the block's threads (in thread order); *total = the block's sum.  Integer sums: the
// result does not depend on the order of the additions.
__device__ __forceinline__ int block_exclusive_scan(int v, int* total) {
    __shared__ int wave_sum[kScanThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int u = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += u;
    }
    if (lane == kWave - 1) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / kWave; ++w) {
        before += (w < wave) ? wave_sum[w] : 0;
        sum += wave_sum[w];
    }
    __syncthreads();                          // (wave_sum is reused by the next call)
    *total = sum;
    return before + incl - v;
}

// Shared underflowing inputs (the predicate: hnrf.h, hnrf_share_compact): the representative's results c_off / c_xyz /
// c_raw, the list of live samples idx[0 .. *count) and the rows the shared samples' results go to.  offsets / xyz
// nullable (the lean form reads neither).  *count must be 0 before the first block runs.
// n raw planes (1..8; the heads of a multi-head canonical image, hnrf_heads_shared.h): c_raw is [n][4], plane g starts
// at raw + g * plane_stride (in float4s) and a shared sample gets c_raw[g] in plane g.  The predicate, the list, offsets
// and xyz do not depend on the head: one of each.
struct ShareOut {
    const float *c_off, *c_xyz, *c_raw;
    int *idx, *count;
    float4* raw;
    float *offsets, *xyz;
    int n = 1;
    int64_t plane_stride = 0;
};

// Sample p with x_skel = x: shared or live (in_range false: neither).  A live sample goes onto the list once (no plane
// row of it is touched); a shared one gets the representative's results, which are its own bit for bit.  PLANES: the
// sh.n planes in a run-time loop, one float4 store each; without it the single plane's code is what it was before
// planes existed (sh.n and sh.plane_stride are not read).
template <bool PLANES = false>
__device__ __forceinline__ void share_classify(bool in_range, int64_t p, const float (&x)[3], const ShareOut& sh) {
#pragma clang fp contract(off)
    bool shared = in_range;
#pragma unroll
    for (int a = 0; a < 3; ++a)        // (a NaN fails the first comparison: always live); the sum is K2's own `x + offset`
        shared &= fabsf(x[a]) <= HNRF_SHARE_T && __float_as_uint(x[a] + sh.c_off[a]) == __float_as_uint(sh.c_xyz[a]);
    const bool keep = in_range && !shared;
    const int slot = block_append(keep, sh.count);
    if (keep) sh.idx[slot] = (int)p;
    if (shared) {
        if constexpr (PLANES) {
            for (int g = 0; g < sh.n; ++g)                                 // (c_raw: wave-uniform addresses, scalar loads)
                sh.raw[(int64_t)g * sh.plane_stride + p] =
                    make_float4(sh.c_raw[4 * g], sh.c_raw[4 * g + 1], sh.c_raw[4 * g + 2], sh.c_raw[4 * g + 3]);
        } else {
            sh.raw[p] = make_float4(sh.c_raw[0], sh.c_raw[1], sh.c_raw[2], sh.c_raw[3]);
        }
        if (sh.offsets) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                sh.offsets[p * 3 + a] = sh.c_off[a];
                sh.xyz[p * 3 + a] = sh.c_xyz[a];
            }
        }
    }
}

}  // namespace hnrf
