/* libhnrf -- training the multi-head canonical MLP: every head through one trunk pass, forward and backward.  Included
 * by hnrf.h (inside its extern "C"); additive to ABI version 13 in the way of hnrf_heads.h: humannerf_amd/_lib.py binds
 * these entries on first use (load_heads_train) and raises when the library lacks them.
 *
 * The network is that of hnrf_heads.h: output_linear.0 is (4 H, 256), head g is its rows 4g .. 4g+3, and the trunk does
 * not know the heads.  The usual convention: raw device pointers, sizes, a stream, int error codes, no allocation, no
 * synchronisation; every entry answers n_heads outside 2..8, a null pointer or a misaligned buffer with HNRF_E_ARG
 * before any launch.
 *
 * ---- hnrf_canonical_heads_fwd_train: hnrf_canonical_fwd_train on the image of hnrf_canonical_heads_pack, with
 *   raw [n_heads][P][4] as hnrf_canonical_heads_fwd writes it.  mode: HNRF_MLP_F32, HNRF_MLP_F16X3 or HNRF_MLP_F16X3_H
 *   (an image packed with HNRF_MLP_F16X3 serves both).  pe_out, acts and relu_bits are those of
 *   hnrf_canonical_fwd_train in the same mode -- shapes, padding rows and columns, the blocked f16 layout -- and equal it
 *   bit for bit on the single-head image of ANY head's four rows; plane g of raw equals that call's raw bit for bit
 *   (per-head descale of the multi-head image, hnrf_heads.h).
 *
 * ---- hnrf_canonical_heads_bwd_packed_bytes / hnrf_canonical_heads_bwd_pack: the transposed image of
 *   hnrf_canonical_bwd_pack whose head stage contracts K = 4 n_heads outputs instead of 4, laid out as the forward's
 *   accumulator holds the heads: head g = 2 q + h on lane half h, so that the chain reads one float4 of d_raw per
 *   (q, half).  weights[8] is (4 n_heads, 256).  mode: HNRF_MLP_F32 or HNRF_MLP_F16X3 (0 bytes / HNRF_E_UNSUPPORTED for
 *   anything else; 0 bytes for n_heads outside 2..8).  Split-f16: the head stage is two k-steps of 16 for every n_heads
 *   (the second one holds zeros up to n_heads = 4), and the head layer's power-of-two lift is taken from the maximum
 *   over ALL heads -- the stage sums over them, so they share one exponent.
 *
 * ---- hnrf_canonical_heads_bwd: hnrf_canonical_bwd seeded with sum_g W_g^T d_raw_g, d_raw [n_heads][P][4] head-major.
 *   Below the head stage it is hnrf_canonical_bwd, and its contracts carry over: dZ [8][P][256] (HNRF_MLP_F16X3_H: the
 *   blocked f16 matrix in the chain's scaled domain with zero padding rows, dz_amax = the 8 scales), d_xyz [P][3],
 *   dz_amax [8][HNRF_AMAX_SLOTS] per-layer maxima (optional in the fp32-dZ modes); d_raw_amax (device scalar, required
 *   in the split-f16 modes) bounds |d_raw| over all planes, the result does not depend on it beyond that bound, a zero
 *   bound gives exact zeros and a non-finite one NaN everywhere; nothing is read before it is written.
 *   HNRF_MLP_F32 and a d_raw that is zero outside plane g: dZ and d_xyz compare equal to hnrf_canonical_bwd on head g's
 *   rows (the other heads contribute exact zero products).
 *
 * The head's own weight gradient needs no entry of its own: hnrf_mlp_dw / hnrf_mlp_dw_h with n_out = 4 once per plane,
 * written to rows 4g .. 4g+3 of the (4 n_heads, 256) gradient through ldw. */
#ifndef HNRF_HEADS_TRAIN_H
#define HNRF_HEADS_TRAIN_H

int hnrf_canonical_heads_fwd_train(const float* xyz, const void* packed, int mode, int64_t P, int n_heads, float* raw,
                                   float* pe_out, float* acts, uint32_t* relu_bits, void* stream);
size_t hnrf_canonical_heads_bwd_packed_bytes(int mode, int n_heads);
int hnrf_canonical_heads_bwd_pack(const float* const* weights, int n_heads, int mode, void* packed, void* stream);
int hnrf_canonical_heads_bwd(const float* xyz, const float* d_raw, const uint32_t* relu_bits, const void* packed, int mode,
                             const float* d_raw_amax, int64_t P, int n_heads, float* dZ, float* d_xyz, float* dz_amax,
                             void* stream);

#endif
