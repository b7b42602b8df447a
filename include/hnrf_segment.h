/* libhnrf -- surface records split by body part.  Included by hnrf.h (inside its extern "C"); additive to ABI version
 * 13 in the way of hnrf_cloud.h: humannerf_amd/_lib.py binds these entries on first use (load_segment) and raises when
 * the library lacks them.
 *
 * Restates tools/segment.py:23-49 of the reference: a part of a frame = the records within L1 pixel distance < radius
 * of a record whose arg-max bone belongs to the part.  The usual convention: raw device pointers, sizes, a stream, int
 * error codes, no allocation, no synchronisation; bad arguments are refused before any launch and hnrf_last_error
 * names the argument.  Integer arithmetic and selection only: every output is a pure function of the input, and
 * humannerf_amd/cloud.py (twin_segment, twin_compact) is the numpy form of every statement below.
 *
 * ---- the batch.  rec [total,10] fp32, the records of F frames packed (columns: xyz | rgb | weight max | row | col |
 *   lbs; cloud.surface_records), offsets [F+1] int64 ascending from 0 to total: frame f = rows offsets[f] ..
 *   offsets[f+1].  offsets stay on the device and are not read back: a row outside every frame takes part in nothing
 *   (member 0), and no index formed from them leaves the buffers' sizes as the arguments give them.
 *
 * ---- hnrf_segment_members: member [total] uint32, bit p set iff the record belongs to part p.
 *   bone_masks [B] uint32, 1 <= B <= 32: the parts that bone b seeds (a bone may seed several; up to 32 parts, bit 31
 *   included).  A record whose bone is outside [0, B) or has mask 0 seeds nothing.  Image H x W, 1 <= H, W <= 16384;
 *   1 <= radius <= 64.
 *   Per frame a bitmap seed[H][W] of uint32 in the workspace: seed[r][c] = the OR of the masks of the records at pixel
 *   (r, c) (an integer OR atomic: two records may share a pixel, and the OR does not depend on their order);
 *   member[n] = the OR of seed[r_n + dr][c_n + dc] over |dr| + |dc| < radius, pixels outside the image skipped.
 *   status [1] int32, zeroed, then written by the first of the three launches (0 = fine), OR of
 *     1  a row or column that is not integer-valued (NaN and infinities included),
 *     2  a pixel outside [0, H) x [0, W),
 *     4  a bone that is not integer-valued.
 *   The later launches of this entry, and those of the two entries below when given the same word, read it on the
 *   device and write NOTHING when it is not 0: nothing is truncated silently, and the host reads the word back with
 *   the counts.
 *   workspace: hnrf_segment_workspace_bytes(F, H, W) = F H W 4 bytes rounded up to 256 (0 for sizes refused), 256-byte
 *   aligned; the host splits a long run into batches of frames.
 *
 * ---- hnrf_segment_count / hnrf_segment_scatter: the stable compaction per (part, frame), P parts (1 <= P <= 32).
 *   A record n is kept in part p iff bit p of member[n] is set and (weight_rec null or weight_rec[10 n + 6] >
 *   weight_min; a NaN weight is not kept).
 *   seg_offsets [P F + 1] int64, part-major: segment p F + f = the kept records of frame f in part p, rows
 *   seg_offsets[p F + f] .. seg_offsets[p F + f + 1] of src; seg_offsets[P F] = the number of rows of src.
 *   src [src_rows] int32: the packed input row of every kept record, ascending within a segment (and so within a
 *   part: the frames lie in order).  hnrf_segment_count writes seg_offsets and leaves the per-block bases in the
 *   workspace; the host reads seg_offsets[P F], sizes src, and hnrf_segment_scatter -- same arguments, same workspace,
 *   untouched in between -- fills it.  A row that would fall at or past src_rows is not written.
 *   Blocks of 256 packed rows: per block and part a count (wave ballots), one exclusive scan over [part][block]
 *   (hnrf_block_scan.h), then every kept record's rank inside its block.
 *   workspace: hnrf_segment_compact_workspace_bytes(total, P) (0 for sizes refused), 256-byte aligned.
 *   total <= 2^31 - 512.  status nullable. */
size_t hnrf_segment_workspace_bytes(int n_frames, int H, int W);
int hnrf_segment_members(const float* rec, const int64_t* offsets, int n_frames, int64_t total,
                         const uint32_t* bone_masks, int n_bones, int H, int W, int radius, void* workspace,
                         size_t workspace_bytes, uint32_t* member, int* status, void* stream);
size_t hnrf_segment_compact_workspace_bytes(int64_t total, int n_parts);
int hnrf_segment_count(const uint32_t* member, const float* weight_rec, float weight_min, const int64_t* offsets,
                       int n_frames, int64_t total, int n_parts, const int* status, void* workspace,
                       size_t workspace_bytes, int64_t* seg_offsets, void* stream);
int hnrf_segment_scatter(const uint32_t* member, const float* weight_rec, float weight_min, int64_t total, int n_parts,
                         const int* status, const void* workspace, size_t workspace_bytes, int* src, int64_t src_rows,
                         void* stream);
