// LDS-DMA (global_load_lds_dwordx4: L2 -> LDS without VGPR staging) as the split-f16 MLP kernels (hnrf_mlp_f16.hip) and
// the f16 weight-gradient kernel (hnrf_mlp_bwd.hip) issue and retire it: from inline asm, so that hipcc does not count the
// loads (its own bookkeeping would put s_waitcnt vmcnt(0) in front of the next ds_read and serialise DMA and MFMAs), and
// with a hand-counted s_waitcnt.
#pragma once

namespace hnrf {

// Lane id recomputed where it is needed (2 VALU).  Volatile on purpose: addresses derived
// from a lane id hoisted to kernel entry get spilled, and the reload's compiler-inserted
// s_waitcnt vmcnt(0) would drain the hand-counted DMA queue on every tile.
__device__ __forceinline__ unsigned lane_now() {
    unsigned l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// One 1-KiB LDS-DMA piece: lane l's 16 bytes at gbase + voff(l) land at LDS byte lds_addr + 16 l; retired by
// wait_dma_keep().  This form saves and restores M0 itself (prologues: slab_issue).
__device__ __forceinline__ void dma_piece(const char* gbase, unsigned voff, unsigned lds_addr) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(gbase), "s"(lds_addr)
        : "memory");
}

// The same inside the k-loops, where every instruction of the one wave per SIMD costs ~5 cycles of issue next to the
// MFMAs' 32 (profiles/tools/mfma_issue.hip: 8 + 5 n cycles per MFMA with n other instructions of ANY kind, scalar ones
// included): the form above is 8 instructions per piece (m0 saved / set / restored, s_nop, two-word source add, LDS
// address add), 1.3 per MFMA of the canonical kernel.  The instruction's immediate offset applies to BOTH addresses
// (LDS address = M0 + offset + 16 lane, measured: profiles/tools/dma_offset.hip), so four consecutive 1-KiB pieces
// share one source base and one M0 value (offsets 0 / 1024 / 2048 / 3072); M0 is handed to the compiler as an operand
// ("{m0}": it materialises the value and the hazard wait itself, and nothing else in these kernels uses M0).
// A wave therefore moves CONTIGUOUS runs of pieces, not every fourth piece of a slab.
template <int R>
__device__ __forceinline__ void dma_piece_g(const char* gbase, unsigned voff, unsigned lds_addr) {
    // a scalar write of M0 needs one wait state before an LDS-DMA instruction reads it (gfx9 hazard), and hipcc, which
    // places the write, cannot see into the asm to insert it: hence the s_nop inside the statement.  In EVERY piece, not
    // only a run's first: where the pieces of a run sit in different basic blocks (runtime piece counts at layer
    // boundaries) the compiler writes M0 again in front of later pieces (the same value, so a stale read would be
    // harmless -- but that is an argument about today's code generation, not a guarantee)
    asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 offset:%3" : : "v"(voff), "s"(gbase), "{m0}"(lds_addr), "n"(R * 1024) : "memory");
}
// piece i (compile-time after unrolling) of this wave's run: base addresses of the wave's run in, group of four out
__device__ __forceinline__ void dma_run_piece(const char* run_src, unsigned voff, unsigned run_dst, int i) {
    const char* g = run_src + (i >> 2) * 4096;
    const unsigned d = run_dst + (i >> 2) * 4096;
    switch (i & 3) {
        case 0: dma_piece_g<0>(g, voff, d); break;
        case 1: dma_piece_g<1>(g, voff, d); break;
        case 2: dma_piece_g<2>(g, voff, d); break;
        default: dma_piece_g<3>(g, voff, d); break;
    }
}
// a whole run of NP pieces at once
template <int NP>
__device__ __forceinline__ void dma_run(const char* gbase, unsigned voff, unsigned lds_addr) {
    static_assert(NP == 2 || NP == 4, "pieces per run");
    dma_piece_g<0>(gbase, voff, lds_addr);
    dma_piece_g<1>(gbase, voff, lds_addr);
    if (NP == 4) {
        dma_piece_g<2>(gbase, voff, lds_addr);
        dma_piece_g<3>(gbase, voff, lds_addr);
    }
}

// wait until at most `keep` of this wave's DMA pieces are still in flight.  For a `keep` that is a compile-time constant
// after inlining (one s_waitcnt); a runtime value is lowered to a compare chain over the whole case list, which is why
// mlp_dwh_dma_kernel keeps a short list of its own (dwh_wait_keep)
__device__ __forceinline__ void wait_dma_keep(int keep) {
#define HNRF_VMCNT_CASE(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    switch (keep) {
        // (even counts: four waves per workgroup; the odd ones: eight, 2 or 3 pieces per wave and slab.  Training variants:
        // the 4 activation stores per finished tile sit in the same in-order queue)
        HNRF_VMCNT_CASE(1) HNRF_VMCNT_CASE(2) HNRF_VMCNT_CASE(3) HNRF_VMCNT_CASE(4) HNRF_VMCNT_CASE(5) HNRF_VMCNT_CASE(6)
        HNRF_VMCNT_CASE(7) HNRF_VMCNT_CASE(8) HNRF_VMCNT_CASE(9) HNRF_VMCNT_CASE(10) HNRF_VMCNT_CASE(11) HNRF_VMCNT_CASE(12)
        HNRF_VMCNT_CASE(13) HNRF_VMCNT_CASE(14) HNRF_VMCNT_CASE(15) HNRF_VMCNT_CASE(16) HNRF_VMCNT_CASE(18) HNRF_VMCNT_CASE(20)
        HNRF_VMCNT_CASE(22) HNRF_VMCNT_CASE(24) HNRF_VMCNT_CASE(26) HNRF_VMCNT_CASE(28) HNRF_VMCNT_CASE(30)
        HNRF_VMCNT_CASE(32) HNRF_VMCNT_CASE(34) HNRF_VMCNT_CASE(36) HNRF_VMCNT_CASE(38) HNRF_VMCNT_CASE(40)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef HNRF_VMCNT_CASE
}

}  // namespace hnrf
