/* libhnrf -- surface-point records and the frame x frame appearance distance.  Included by hnrf.h (inside its
 * extern "C"); additive to ABI version 13: a library built before these entries existed lacks the symbols and nothing
 * else changes, so humannerf_amd/_lib.py binds them on first use (load_cloud) and raises when they are missing.
 *
 * Restates run.py:388-404 (cfg.test.save_3d_together: one canonical surface point per ray) and
 * tools/compute_distance*.py (find_nearest_pair_gpu / compute_distance_gpu) of the reference.  The usual convention:
 * raw device pointers, sizes, a stream, int error codes, no allocation, no synchronisation; bad shapes are refused
 * before anything is launched.  humannerf_amd/cloud.py holds the numpy twin of every statement below.
 *
 * ---- the arithmetic, used by every entry and by the twin (no contraction, correctly rounded sqrt):
 *   d2(a, b) = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)),  dx = fl(ax - bx), fp32;
 *   the nearest neighbour of a in a cloud = the candidate of smallest d2, ties to the LOWEST ORIGINAL RECORD INDEX
 *   (what torch.argmin returns on the CPU); a candidate whose d2 is NaN never wins;
 *   a distance = fl(sqrt(d2)); the colour error of two points = the same expression on their rgb columns.
 *   (torch.linalg.norm is not bit-equal to it: parity with the reference is a statement about decisions,
 *   tests/test_cloud_refs.py.)
 *
 * ---- hnrf_surface_points: run.py:391-396.
 *   weights [R,S], xyz [R,S,3], bmw [R,S,B] (weights_on_rays, xyz_on_rays, backward_motion_weights of the frame entries)
 *   -> wxyz [R,3] = sum_s w xyz, wmax [R] = max_s w, lbs [R] int32 = the lowest-index argmax over b of sum_s w bmw[s,b].
 *   One wave per ray.  fp32 sums in one fixed order: lane l adds the samples l, l + 64, l + 128, ... ascending
 *   (acc = fl(acc + fl(w x)) from 0), then the 64 lanes are added by a butterfly over the lane distances 32, 16, 8, 4,
 *   2, 1 -- a ray's values depend on S alone, not on R, its row or the launch.
 *   R >= 0 (0 launches nothing and the pointers are not looked at), 1 <= S <= 512, 1 <= B <= 32 (HNRF_E_UNSUPPORTED
 *   beyond; HNRF_E_ARG below).
 *
 * ---- hnrf_cloud_nn: brute force, the counterpart of find_nearest_pair_gpu's argmin and the oracle of the windowed entry.
 *   a [Na,3], b [Nb,3] -> idx [Na] int32 = the nearest neighbour in b, d2 [Na] its d2.  Cloud b goes through LDS in
 *   tiles and is walked in index order.  Nb = 0: idx = -1, d2 = +inf.  Na = 0 launches nothing.  Nothing is written
 *   past Na.  Na, Nb < 2^31.
 *
 * ---- hnrf_cloud_distance_pairs: D[p] = the appearance distance of the frames pairs[p] = (i, j), for P pairs at once.
 *   Packed clouds of F frames: xyz [total,3], rgb [total,3], orig [total] int32 (a point's record index inside its
 *   frame: the tie-break, and what `match` reports), offsets [F+1] int64 (frame f = rows offsets[f] .. offsets[f+1]);
 *   each frame's rows are sorted ascending by coordinate `axis` (0, 1, 2).  pairs [P,2] int32.  tau = dist_thresh,
 *   finite and > 0 (anything else: HNRF_E_ARG before any launch).  max_n >= every frame's count, <= 2^24.
 *   Per point p of frame i:
 *     1 the window of frame j: the q with |k_p - k_q| <= tau (1 + 2^-20), k = coordinate `axis`; the two bounds
 *       k_p -+ tau (1 + 2^-20) are formed and compared in fp64, located by binary search;
 *     2 q = the argmin of d2(p, .) over the window, ties by orig;
 *     3 if the window is not empty and fl(sqrt(d2(p, q))) < tau: the same search from q in frame i;
 *     4 where that returns p, D gains the colour error of (p, q) and match[p] = orig[q].
 *   d < tau implies |k_p - k_q| <= d (1 + 3 2^-24) < tau (1 + 2^-20), so the window holds every candidate that can win
 *   and all ties of a sub-tau minimum: the pairs are those of hnrf_cloud_nn both ways, filtered by d < tau, point for
 *   point.  The kernel searches, for the 256 points of a workgroup (neighbours along the sort
 *   coordinate), the UNION of their windows, staged through LDS: any superset of a point's window gives the same
 *   match and D, because what it adds is farther than tau.
 *   D [P] float64: each workgroup (256 points of frame i) adds its contributions in thread order -- lane 16 g the
 *   lanes 16 g .. 16 g + 15 ascending, then lane 0 the 16 groups ascending -- and a second kernel adds a pair's
 *   partials in block order.  No atomics: bit-reproducible, and D[p] depends on pairs[p] alone.
 *   match (nullable) [P][max_n] int32: per SORTED position of frame i the partner's orig, -1 for no partner and for
 *   positions past the frame's count.
 *   A pair naming a frame outside [0, F), or a frame whose rows do not lie inside [0, total] or exceed max_n, counts as
 *   an empty frame (D = 0): offsets and pairs live on the device and are not read back.
 *   workspace: hnrf_cloud_distance_pairs_workspace_bytes(P, max_n) bytes (0 for sizes refused), 256-byte aligned.  The
 *   host side launches the pairs in chunks of 65535 (the grid limit) that reuse it in stream order. */
int hnrf_surface_points(const float* weights, const float* xyz, const float* bmw, int64_t R, int S, int B, float* wxyz,
                        float* wmax, int* lbs, void* stream);
int hnrf_cloud_nn(const float* a, int64_t Na, const float* b, int64_t Nb, int* idx, float* d2, void* stream);
size_t hnrf_cloud_distance_pairs_workspace_bytes(int64_t n_pairs, int64_t max_n);
int hnrf_cloud_distance_pairs(const float* xyz, const float* rgb, const int* orig, const int64_t* offsets, int n_frames,
                              int64_t total, const int* pairs, int64_t n_pairs, int64_t max_n, int axis, float tau,
                              void* workspace, size_t workspace_bytes, double* D, int* match, void* stream);
