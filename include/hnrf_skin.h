/* libhnrf -- bone weights as data, and the skinning a glTF viewer performs: the device side of the skinned glTF export
 * (humannerf_amd/gltf.py, run.run_gltf).  Included by hnrf.h (inside its extern "C"); additive to ABI version 13:
 * humannerf_amd/_lib.py binds these entries on first use (load_skin) and raises when the library lacks them.
 *
 * The usual convention: raw device pointers, sizes, a stream, int error codes, no allocation, no synchronisation; bad
 * arguments are refused before any launch and hnrf_last_error names the argument.  One thread per vertex, no atomics:
 * every output is a pure function of the input.  All arithmetic is fp32, every operation rounded on its own (no fma,
 * IEEE division), in the order stated below; humannerf_amd/skin.py (skin_weights_host, skin_lbs_host) is the numpy form
 * of every statement, bit for bit.  V >= 0 (V = 0: nothing is launched, the pointers are not looked at).
 *
 * ---- hnrf_skin_weights: the K largest bone weights of every vertex, normalised.  K = 4 or 8, 1 <= B <= 128, G as
 *   hnrf_forward_skin.  verts [V,3]; vol [>=B,G,G,G] (the first B channels are read); bbox_min, bbox_scale [3].
 *   w_b = the weight hnrf_forward_skin blends with -- the same device function (csrc/hnrf_trilinear.h): trilinear,
 *     align_corners, zero padding; w = 0, then w = w + vol[b][corner k] * c_k for the corners k = 0..7 (x fastest).  A
 *     NaN coordinate samples as zero-padded: every corner weight is 0.
 *   Selection: K slots (s_k, j_k), all (0, 0) at first.  The bones are visited in ascending b; bone b enters in front of
 *     the first slot with w_b > s_k, and the slots from there on move down one place (the last drops out).  So the
 *     slots hold the K largest POSITIVE weights in descending order, equal weights in ascending bone order; a weight
 *     that is 0, negative or NaN is never selected, and a slot that nothing entered stays (0, joint 0) -- fewer than K
 *     bones, or fewer than K positive weights.
 *   kept = ((s_0 + s_1) + s_2) + ... + s_{K-1}.
 *   kept > 0:  joints[k] = j_k, weights[k] = s_k / kept.
 *   otherwise (every corner zero-padded, a NaN coordinate, an all-zero volume): joints all 0, weights (1, 0, ..., 0).
 *   joints [V,K] uint8, 4-byte aligned; weights [V,K] fp32, 16-byte aligned; kept [V] fp32, nullable.
 *
 * ---- hnrf_skin_lbs: out [V,3] = sum_k weights[k] (mats[joints[k]] (x, 1)), the arithmetic of glTF skinning with
 *   mats[b] = the joint matrix of bone b ([B,3,4] row-major: the upper three rows of world(joint b) * inverseBind(b)).
 *   K = 4 or 8, 1 <= B <= 128.  acc = (0, 0, 0); for k = 0 .. K-1 in order, with m = mats[joints[k]]:
 *     p_i = ((m[i][0] * x + m[i][1] * y) + m[i][2] * z) + m[i][3];   acc_i = acc_i + weights[k] * p_i.
 *   A slot whose joint index is >= B is skipped (its weight is not read into the sum).  Alignment of joints and weights
 *   as above. */
int hnrf_skin_weights(const float* verts, int64_t V, const float* vol, int B, int G, const float* bbox_min,
                      const float* bbox_scale, int K, uint8_t* joints, float* weights, float* kept, void* stream);
int hnrf_skin_lbs(const float* verts, int64_t V, const uint8_t* joints, const float* weights, int K, const float* mats,
                  int B, float* out, void* stream);
