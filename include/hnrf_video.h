/* libhnrf -- baseline JPEG encoding of 8-bit RGB images on the device (the frames of a Motion-JPEG video).  Included by
 * hnrf.h (inside its extern "C"); additive to ABI version 13: a library built before these entries existed lacks the
 * symbols and nothing else changes, so humannerf_amd/_lib.py binds them on first use (load_video) and raises when they
 * are missing.  The usual convention: raw device pointers, sizes, a stream, int error codes, no allocation, no
 * synchronisation; bad arguments are refused before anything is launched.  humannerf_amd/video.py holds the numpy twin
 * (jpeg_encode_numpy), which writes the same bytes; DESIGN.md section 4 "Video" states the format.
 *
 * ---- the stream: baseline sequential JPEG (SOF0), 8 bit, JFIF APP0, YCbCr full-range BT.601, 4:2:0; an MCU is 16 x 16
 *   pixels (Y00 Y01 Y10 Y11 Cb Cr), the image is padded right / bottom to multiples of 16 by edge replication; Annex-K
 *   quantisation tables scaled by the usual quality rule (s = 5000 / q below 50, else 200 - 2 q; clip((base s + 50) / 100,
 *   1, 255)), the four Annex-K Huffman tables; DRI = 1: every MCU is coded alone from DC predictors 0 (Y01 predicts from
 *   Y00, Y10 from Y01, Y11 from Y10), padded with 1-bits to a byte, byte-stuffed, followed by RST(n & 7), the last by EOI.
 * ---- the arithmetic, integer only (>> = arithmetic shift):
 *   Y  = (19595 R + 38470 G + 7471 B + 2^15) >> 16 per pixel;  with Rs, Gs, Bs the sums over a 2 x 2 quad
 *   Cb = clip((-11058 Rs - 21710 Gs + 32768 Bs + 128 2^18 + 2^17) >> 18, 0, 255),
 *   Cr = clip(( 32768 Rs - 27439 Gs -  5329 Bs + 128 2^18 + 2^17) >> 18, 0, 255);  s = sample - 128;
 *   C[k][n] = round(2^14 c_k cos((2n + 1) k pi / 16)), c_0 = sqrt(1/8), c_k = 1/2;
 *   t[y][u] = (sum_x C[u][x] s[y][x] + 2^9) >> 10;  F[v][u] = (sum_y C[v][y] t[y][u] + 2^17) >> 18  (int32 throughout);
 *   k = sign(F) ((2 |F| + Q) / (2 Q)), then DC clipped to [-1024, 1023], AC to [-1023, 1023].
 *
 * ---- hnrf_jpeg_header (host): the bytes in front of the first MCU (SOI, APP0, DQT, SOF0, DHT, DRI, SOS) for an H x W
 *   image at `quality`, into host_out[0 .. cap); returns their number (613), or a negative error code (sizes outside
 *   1 .. 65535, quality outside 1 .. 100, cap too small).  The caller uploads them once per (H, W, quality).
 * ---- hnrf_jpeg_encode: rgb = device pointer of pixel (0, 0), pixel (y, x) at rgb + y row_stride + 3 x (row_stride >= 3 W
 *   bytes); only the 3 W bytes of each of the H rows are read, so a buffer of (H - 1) row_stride + 3 W bytes is enough:
 *   the padding behind the last row need not exist.  header / header_len = the uploaded header (device memory,
 *   header_len <= 1024; exactly header_len bytes are read).  Three launches on `stream`:
 *   one wave per MCU (colour transform, six DCTs through LDS, quantisation, Huffman coding by ballot and wave prefix
 *   sum into an LDS bit buffer, byte stuffing) writes the MCU's fixed slot of HNRF_JPEG_SLOT_BYTES in the workspace
 *   and its length; one block scans the lengths; the third kernel copies header, slots and markers into `out` and
 *   writes the stream's length to *out_len.  Nothing beyond out[0 .. *out_len) and *out_len is written outside the
 *   workspace: the bytes of out from *out_len on keep what they held, and out_len is one uint32 (4 bytes).  What the
 *   workspace held before the call does not matter.  Refused before any launch (nothing is written then): sizes
 *   outside 1 .. 65535, quality outside 1 .. 100, null pointers (HNRF_E_ARG);
 *   an image whose hnrf_jpeg_max_bytes does not fit the uint32 length word (HNRF_E_UNSUPPORTED: about 1.7 million MCUs);
 *   workspace_bytes < hnrf_jpeg_workspace_bytes or out_cap < hnrf_jpeg_max_bytes (HNRF_E_WORKSPACE).  workspace must be
 *   256-byte aligned, out_len 4-byte aligned.
 * ---- hnrf_jpeg_workspace_bytes / hnrf_jpeg_max_bytes: 0 for sizes outside 1 .. 65535.  max_bytes = 1024 for the header
 *   + (slot + 2 marker bytes) per MCU: the worst case, not what a picture takes. */
#define HNRF_JPEG_SLOT_BYTES 2496
size_t hnrf_jpeg_workspace_bytes(int H, int W);
size_t hnrf_jpeg_max_bytes(int H, int W);
int hnrf_jpeg_header(int H, int W, int quality, uint8_t* host_out, int cap);
int hnrf_jpeg_encode(const uint8_t* rgb, int H, int W, int64_t row_stride, const uint8_t* header, int header_len, int quality,
                     void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_cap, uint32_t* out_len, void* stream);
