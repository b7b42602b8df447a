"""Motion-JPEG output of the render loops: a baseline JPEG encoder (numpy twin of csrc/hnrf_video.hip, bit for bit),
its device binding, and the RIFF AVI container (DESIGN.md section 4 "Video", include/hnrf_video.h).

  jpeg_encode_numpy   the twin: the stream format stated once below, in integer arithmetic
  JpegEncoder         .encode(rgb8 device tensor) -> (device byte buffer, length word), nothing synchronises
  MjpegWriter         .add(name, jpeg bytes) / .finalize(): RIFF AVI, 'MJPG' video stream, idx1, frames sorted by name
  merge_parts         the per-rank files of a frame-sharded run interleaved into one, no re-encoding

The stream: baseline sequential JPEG (SOF0), 8 bit, JFIF APP0, YCbCr full-range BT.601, 4:2:0, one MCU = 16 x 16 pixels
(Y00 Y01 Y10 Y11 Cb Cr), the image padded right / bottom to multiples of 16 by edge replication, Annex-K quantisation
tables scaled by the usual quality rule, the four Annex-K Huffman tables, DRI = 1: every MCU is coded alone (DC
predictors 0 at its start), padded with 1-bits to a byte, byte-stuffed, and followed by RST(n & 7) -- EOI after the last.

The arithmetic (all integer; >> is the arithmetic shift = floor):
  Y        = (19595 R + 38470 G + 7471 B + 2^15) >> 16                                        per pixel
  Cb       = clip((-11058 Rs - 21710 Gs + 32768 Bs + 128 * 2^18 + 2^17) >> 18, 0, 255)        Rs, Gs, Bs = sums over the 2 x 2 pixels
  Cr       = clip(( 32768 Rs - 27439 Gs -  5329 Bs + 128 * 2^18 + 2^17) >> 18, 0, 255)        (mean and transform in one rounding)
  s        = sample - 128
  C[k][n]  = round(2^14 c_k cos((2n + 1) k pi / 16)),  c_0 = sqrt(1/8), c_k = 1/2             DCT_MATRIX below
  rows     t[y][u] = (sum_x C[u][x] s[y][x] + 2^9) >> 10          (4 fractional bits kept; |t| <= 8192)
  columns  F[v][u] = (sum_y C[v][y] t[y][u] + 2^17) >> 18         (|sum| < 2^30: int32 throughout)
  quantise k = sign(F) ((2 |F| + Q) // (2 Q))  (round half away from zero), then DC clipped to [-1024, 1023] and AC to
           [-1023, 1023]: the size categories that baseline Huffman tables hold (DC difference <= 11, AC <= 10)
"""
import os
import struct

import numpy as np

# ------------------------------------------------------------------------------------------------ tables (ITU-T T.81 Annex K)
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
    80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
    95, 98, 112, 100, 103, 99], dtype=np.int64)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
    99, 99] + [99] * 32, dtype=np.int64)
# ZIGZAG[j] = the natural (row-major) index of the j-th coefficient of the scan
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
    42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
    63], dtype=np.int64)
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
    0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
    0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
    0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
    0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
    0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
    0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
    0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa]

# round(2^14 c_k cos((2n + 1) k pi / 16)): written out, because the kernel holds the same 64 integers
DCT_MATRIX = np.array([
    [5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793],
    [8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035],
    [7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568],
    [6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811],
    [5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793],
    [4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551],
    [3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135],
    [1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598]], dtype=np.int64)

# One MCU's slot in the encoder's workspace, a derived worst case: 6 blocks x (DC: 9-bit code + 11 amplitude bits, plus
# 63 coefficients x (16-bit code + 10 amplitude bits)) = 9948 bits = 1244 bytes once padded to a byte, doubled because
# every byte may be an FF that is stuffed, rounded up to a multiple of 64 bytes.
SLOT_BYTES = 2496
HEADER_MAX = 1024               # what hnrf_jpeg_max_bytes allows for the header (it is 613 bytes long)


def slot_bound():
    bits = 6 * ((9 + 11) + 63 * (16 + 10))
    return -(-(2 * -(-bits // 8)) // 64) * 64


def huff_table(bits, vals):
    """(code, length) arrays over the 256 symbols, lengths 0 where a symbol has no code (T.81 Annex C)."""
    code, size = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    c, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code[vals[k]], size[vals[k]] = c, length
            c += 1
            k += 1
        c <<= 1
    return code, size


_DC = (huff_table(DC_LUMA_BITS, DC_VALS), huff_table(DC_CHROMA_BITS, DC_VALS))
_AC = (huff_table(AC_LUMA_BITS, AC_LUMA_VALS), huff_table(AC_CHROMA_BITS, AC_CHROMA_VALS))


def quant_tables(quality):
    """(luma, chroma) int64 [64] in natural order: clip((base s + 50) // 100, 1, 255), s = 5000 // q below 50, else
    200 - 2 q -- what PIL.Image.save(quality=q) writes."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError('JPEG quality must be in 1..100, got %r' % (quality,))
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((b * s + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA))


def jpeg_header(height, width, quality):
    """Everything in front of the first MCU: SOI, APP0 (JFIF 1.1, no density), DQT 0 and 1, SOF0, the four DHT, DRI = 1,
    SOS.  hnrf_jpeg_header writes the same bytes."""
    if not (1 <= height <= 65535 and 1 <= width <= 65535):
        raise ValueError('JPEG sizes are 1..65535 per side, got %d x %d' % (height, width))
    ql, qc = quant_tables(quality)
    seg = lambda marker, body: bytes([0xFF, marker]) + struct.pack('>H', len(body) + 2) + body
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\0\x01\x01\0\0\x01\0\x01\0\0')
    out += seg(0xDB, bytes([0]) + bytes(ql[ZIGZAG].tolist()) + bytes([1]) + bytes(qc[ZIGZAG].tolist()))
    out += seg(0xC0, struct.pack('>BHHB', 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    dht = b''
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        dht += bytes([tc_th]) + bytes(bits) + bytes(vals)
    out += seg(0xC4, dht) + seg(0xDD, struct.pack('>H', 1))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def _bit_length(a):
    """Size category of |a| <= 2047: the number of bits of the magnitude."""
    n = np.zeros(a.shape, dtype=np.int64)
    for k in range(11):
        n += a >= (1 << k)
    return n


def mcu_coefficients(rgb8, quality):
    """The quantised coefficients [n_mcu, 6, 64] (int64, zig-zag order, DC not yet differenced) of an (H, W, 3) uint8
    image, MCUs in raster order."""
    a = np.asarray(rgb8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('jpeg_encode_numpy takes a uint8 image (H, W, 3)')
    H, W = a.shape[:2]
    my, mx = -(-H // 16), -(-W // 16)
    p = np.pad(a, ((0, my * 16 - H), (0, mx * 16 - W), (0, 0)), mode='edge').astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    quad = lambda c: c.reshape(my * 8, 2, mx * 8, 2).sum(axis=(1, 3))
    Rs, Gs, Bs = quad(R), quad(G), quad(B)
    Cb = np.clip((-11058 * Rs - 21710 * Gs + 32768 * Bs + (128 << 18) + (1 << 17)) >> 18, 0, 255)
    Cr = np.clip((32768 * Rs - 27439 * Gs - 5329 * Bs + (128 << 18) + (1 << 17)) >> 18, 0, 255)
    yb = Y.reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my * mx, 4, 8, 8)       # Y00 Y01 Y10 Y11
    cb = Cb.reshape(my, 8, mx, 8).transpose(0, 2, 1, 3).reshape(my * mx, 1, 8, 8)
    cr = Cr.reshape(my, 8, mx, 8).transpose(0, 2, 1, 3).reshape(my * mx, 1, 8, 8)
    s = np.concatenate([yb, cb, cr], axis=1) - 128                                                  # [n, 6, y, x]
    t = (np.einsum('ux,nbyx->nbyu', DCT_MATRIX, s) + (1 << 9)) >> 10
    F = (np.einsum('vy,nbyu->nbvu', DCT_MATRIX, t) + (1 << 17)) >> 18
    ql, qc = quant_tables(quality)
    Q = np.stack([ql] * 4 + [qc] * 2).reshape(1, 6, 8, 8)
    k = np.sign(F) * ((2 * np.abs(F) + Q) // (2 * Q))
    k = k.reshape(-1, 6, 64)[:, :, ZIGZAG]
    k[:, :, 0] = np.clip(k[:, :, 0], -1024, 1023)
    k[:, :, 1:] = np.clip(k[:, :, 1:], -1023, 1023)
    return k


def encode_mcus(coef):
    """Entropy-code MCUs: ``coef`` [n, 6, 64] from mcu_coefficients.  Returns (list of n byte strings: padded to a byte
    and stuffed, no marker; counters {'zrl', 'eob_absent', 'stuffed', 'max_dc_diff'})."""
    n = coef.shape[0]
    v = coef.copy()
    v[:, 1:4, 0] = coef[:, 1:4, 0] - coef[:, 0:3, 0]                  # Y01 from Y00, ...; Y00, Cb, Cr from 0
    chroma = np.array([0, 0, 0, 0, 1, 1])
    size = _bit_length(np.abs(v))
    amp = np.where(v > 0, v, v + (1 << size) - 1)                     # (0 for v == 0: size 0)
    j = np.arange(64).reshape(1, 1, 64)
    nz = v != 0
    nz[:, :, 0] = True
    last = np.maximum.accumulate(np.where(nz, j, 0), axis=2)          # the last coded position at or before j
    prev = np.concatenate([np.zeros_like(last[:, :, :1]), last[:, :, :-1]], axis=2)
    run = j - prev - 1
    # symbols: [n, 6, 65] values and lengths (position 64 = EOB)
    val = np.zeros((n, 6, 65), dtype=np.uint64)
    length = np.zeros((n, 6, 65), dtype=np.int64)
    n_zrl = 0
    for c in (0, 1):
        blocks = np.nonzero(chroma == c)[0]
        dcc, dcs = _DC[c]
        acc, acs = _AC[c]
        vv, ss, aa = v[:, blocks], size[:, blocks], amp[:, blocks]
        # DC
        val[:, blocks, 0] = ((dcc[ss[:, :, 0]] << ss[:, :, 0]) | aa[:, :, 0]).astype(np.uint64)
        length[:, blocks, 0] = dcs[ss[:, :, 0]] + ss[:, :, 0]
        # AC
        on = (vv != 0)
        on[:, :, 0] = False
        r = np.where(on, run[:, blocks], 0)
        zr, sym = r >> 4, ((r & 15) << 4) | ss
        n_zrl += int(zr[on].sum())
        zc, zs = int(acc[0xF0]), int(acs[0xF0])
        pre = np.zeros(vv.shape, dtype=np.int64)
        for k in (1, 2, 3):
            pre = np.where(zr >= k, (pre << zs) | zc, pre)
        code = (((pre << acs[sym]) | acc[sym]) << ss) | aa
        ln = zr * zs + acs[sym] + ss
        val[:, blocks, 1:64] = np.where(on, code, 0)[:, :, 1:].astype(np.uint64)
        length[:, blocks, 1:64] = np.where(on, ln, 0)[:, :, 1:]
        eob = vv[:, :, 63] == 0
        val[:, blocks, 64] = np.where(eob, acc[0], 0).astype(np.uint64)
        length[:, blocks, 64] = np.where(eob, acs[0], 0)
    counters = {'zrl': n_zrl, 'eob_absent': int((coef[:, :, 63] != 0).sum()),
                'max_dc_diff': int(np.abs(v[:, :, 0]).max()) if n else 0}
    # bit placement: symbol bits, MSB first, behind one another; each MCU padded with 1-bits to a byte
    length = length.reshape(n, -1)
    val = val.reshape(n, -1)
    mcu_bits = length.sum(axis=1)
    mcu_bytes = (mcu_bits + 7) >> 3
    mcu_start = np.concatenate([[0], np.cumsum(mcu_bytes * 8)])       # bit offset of every MCU in the common array
    within = np.cumsum(length, axis=1) - length
    start = (mcu_start[:-1, None] + within).reshape(-1)
    flat_len, flat_val = length.reshape(-1), val.reshape(-1)
    bits = np.ones(int(mcu_start[-1]), dtype=np.uint8)
    sym_of_bit = np.repeat(np.arange(flat_len.size), flat_len)
    first = np.cumsum(flat_len) - flat_len
    k = np.arange(sym_of_bit.size) - first[sym_of_bit]                # the k-th bit of its symbol, from the top
    shift = (flat_len[sym_of_bit] - 1 - k).astype(np.uint64)
    bits[start[sym_of_bit] + k] = ((flat_val[sym_of_bit] >> shift) & np.uint64(1)).astype(np.uint8)
    raw = np.packbits(bits)
    ff = np.nonzero(raw == 0xFF)[0]
    counters['stuffed'] = int(ff.size)
    stuffed = np.insert(raw, ff + 1, 0)
    byte_start = mcu_start >> 3
    byte_start = byte_start + np.searchsorted(ff, byte_start, side='left')       # FFs in front of a position shift it
    data = stuffed.tobytes()
    return [data[byte_start[i]:byte_start[i + 1]] for i in range(n)], counters


def jpeg_encode_numpy(rgb8, quality, counters=None):
    """The stream of the module docstring for an (H, W, 3) uint8 image, as bytes: what hnrf_jpeg_encode writes, byte for
    byte, and what a CPU device uses.  ``counters``: a dict that receives the twin's counts of ZRL codes, blocks without
    EOB, stuffed bytes and the largest |DC difference| (what the tests assert about their images)."""
    a = np.asarray(rgb8)
    coef = mcu_coefficients(a, quality)
    mcus, cnt = encode_mcus(coef)
    if counters is not None:
        counters.update(cnt)
    out = [jpeg_header(a.shape[0], a.shape[1], quality)]
    for i, m in enumerate(mcus):
        out.append(m)
        out.append(bytes([0xFF, 0xD0 + (i & 7)]) if i + 1 < len(mcus) else b'\xff\xd9')
    return b''.join(out)


def jpeg_size(data):
    """(height, width) from the SOF0 segment of a JPEG stream."""
    pos = 2
    while pos + 4 <= len(data) and data[pos] == 0xFF:
        marker, size = data[pos + 1], struct.unpack('>H', data[pos + 2:pos + 4])[0]
        if marker == 0xC0:
            return struct.unpack('>HH', data[pos + 5:pos + 9])
        if marker == 0xDA:
            break
        pos += 2 + size
    raise ValueError('no SOF0 segment in the JPEG stream')


# ------------------------------------------------------------------------------------------------ device encoder
class JpegEncoder:
    """hnrf_jpeg_encode on ``device`` at one ``quality``.  ``encode(rgb8)``: (H, W, 3) uint8 tensor on the device, rows
    may be strided (a column slice of a wider image) -> (uint8 buffer of hnrf_jpeg_max_bytes, int64 tensor [1] holding
    the stream's length); the stream is buffer[:length].  Three launches on the current stream, no allocation inside the
    library and no synchronisation: the workspace and the uploaded header are cached per (H, W), the two results are new
    tensors per call (the caller copies them on another stream while the next frame is encoded).  On a CPU device the
    twin encodes."""

    def __init__(self, device, quality=90):
        import torch
        self.device = torch.device(device)
        self.quality = int(quality)
        quant_tables(self.quality)
        self._cache = {}
        if self.device.type == 'cuda':
            from . import _lib
            self._lib = _lib.load_video()

    def max_bytes(self, H, W):
        if self.device.type != 'cuda':
            return HEADER_MAX + (-(-H // 16)) * (-(-W // 16)) * (SLOT_BYTES + 2)
        return int(self._lib.hnrf_jpeg_max_bytes(H, W))

    def _shape_state(self, H, W):
        import ctypes
        import torch
        hit = self._cache.get((H, W))
        if hit is None:
            host = (ctypes.c_uint8 * HEADER_MAX)()
            n = self._lib.hnrf_jpeg_header(H, W, self.quality, host, HEADER_MAX)
            if n <= 0:
                from ._lib import check
                check(n, 'hnrf_jpeg_header')
            header = torch.frombuffer(bytearray(host)[:n], dtype=torch.uint8).to(self.device)
            ws_bytes = int(self._lib.hnrf_jpeg_workspace_bytes(H, W))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            hit = self._cache[(H, W)] = (header, n, ws, ws_bytes, int(self._lib.hnrf_jpeg_max_bytes(H, W)))
        return hit

    def encode(self, rgb8):
        import torch
        if rgb8.dtype != torch.uint8 or rgb8.dim() != 3 or rgb8.shape[2] != 3:
            raise ValueError('JpegEncoder.encode takes a uint8 tensor (H, W, 3)')
        H, W = int(rgb8.shape[0]), int(rgb8.shape[1])
        if self.device.type != 'cuda':
            data = jpeg_encode_numpy(rgb8.cpu().numpy(), self.quality)
            return torch.frombuffer(bytearray(data), dtype=torch.uint8), torch.tensor([len(data)], dtype=torch.int64)
        from ._lib import check
        if rgb8.device != self.device:
            raise ValueError('JpegEncoder.encode: the image is on %s, the encoder on %s' % (rgb8.device, self.device))
        if H < 1 or W < 1 or rgb8.stride(2) != 1 or rgb8.stride(1) != 3 or (H > 1 and rgb8.stride(0) < 3 * W):
            rgb8 = rgb8.contiguous()
        header, n, ws, ws_bytes, cap = self._shape_state(H, W)
        out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        length = torch.zeros(1, dtype=torch.int64, device=self.device)          # (the kernel writes its low uint32)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(self._lib.hnrf_jpeg_encode(rgb8.data_ptr(), H, W, int(rgb8.stride(0)) if H > 1 else 3 * W, header.data_ptr(), n,
                                         self.quality, ws.data_ptr(), ws_bytes, out.data_ptr(), cap, length.data_ptr(),
                                         stream), 'hnrf_jpeg_encode')
        return out, length


# ------------------------------------------------------------------------------------------------ container
RIFF_LIMIT = (1 << 31) - 1


def _chunk(fourcc, body):
    return fourcc + struct.pack('<I', len(body)) + body + (b'\0' if len(body) & 1 else b'')


def _avi_bytes(width, height, fps, frames):
    """The whole file for ``frames`` (a list of JPEG byte strings, in playing order)."""
    n = len(frames)
    biggest = max([len(f) for f in frames] + [0])
    total = sum(8 + len(f) + (len(f) & 1) for f in frames)
    if 12 + 8 + 4 + 64 + 8 + 4 + 64 + 48 + 12 + total + 8 + 16 * n > RIFF_LIMIT:
        return None
    avih = struct.pack('<14I', int(round(1e6 / fps)), int(biggest * fps), 0, 0x10, n, 0, 1, biggest, width, height, 0, 0, 0, 0)
    strh = b'vids' + b'MJPG' + struct.pack('<IHHIIIIIIII4H', 0, 0, 0, 0, 1, int(fps), 0, n, biggest, 0xFFFFFFFF, 0,
                                           0, 0, width, height)
    strf = struct.pack('<IiiHH4sIiiII', 40, width, height, 1, 24, b'MJPG', width * height * 3, 0, 0, 0, 0)
    strl = b'LIST' + struct.pack('<I', 4 + 8 + len(strh) + 8 + len(strf)) + b'strl' + _chunk(b'strh', strh) + _chunk(b'strf', strf)
    hdrl_body = b'hdrl' + _chunk(b'avih', avih) + strl
    hdrl = b'LIST' + struct.pack('<I', len(hdrl_body)) + hdrl_body
    movi, idx, off = [b'movi'], [], 4
    for f in frames:
        idx.append(b'00dc' + struct.pack('<III', 0x10, off, len(f)))            # AVIIF_KEYFRAME; offset from 'movi'
        c = _chunk(b'00dc', f)
        movi.append(c)
        off += len(c)
    movi = b''.join(movi)
    body = b'AVI ' + hdrl + b'LIST' + struct.pack('<I', len(movi)) + movi + _chunk(b'idx1', b''.join(idx))
    return b'RIFF' + struct.pack('<I', len(body)) + body


class MjpegWriter:
    """Motion-JPEG in a RIFF AVI: ``hdrl`` (``avih``, one ``strl`` with ``strh`` 'vids' / 'MJPG' and ``strf`` = a
    BITMAPINFOHEADER with biCompression 'MJPG'), ``movi`` with one even-padded ``00dc`` chunk per frame, ``idx1``.
    ``add(name, jpeg_bytes)`` in any order; ``finalize()`` writes the frames sorted by name (as the reference's
    ImageWriter.finalize sorts them) plus ``<path>.names.txt``, one name per line in that order (what merge_parts
    reads), and returns the path.  ``fps`` is an integer >= 1 (10 as in the reference).  A file past the 2 GiB RIFF
    limit is refused with a ValueError that names it, and nothing is written."""

    def __init__(self, path, width, height, fps=10):
        if isinstance(fps, bool) or not isinstance(fps, int) or fps < 1:
            raise ValueError('MjpegWriter: fps must be an integer >= 1, got %r' % (fps,))
        if not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
            raise ValueError('MjpegWriter: sizes are 1..65535 per side, got %r x %r' % (width, height))
        self.path, self.width, self.height, self.fps = path, int(width), int(height), fps
        self.frames = {}

    def add(self, name, jpeg_bytes):
        name = str(name)
        if name in self.frames:
            raise ValueError('MjpegWriter: frame %r added twice' % name)
        if '\n' in name:
            raise ValueError('MjpegWriter: a frame name holds a line break')
        self.frames[name] = bytes(jpeg_bytes)

    def finalize(self):
        names = sorted(self.frames)
        data = _avi_bytes(self.width, self.height, self.fps, [self.frames[k] for k in names])
        if data is None:
            raise ValueError('%s: %d frames pass the 2 GiB limit of a RIFF file (OpenDML is not written)'
                             % (self.path, len(names)))
        os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
        with open(self.path, 'wb') as f:
            f.write(data)
        with open(self.path + '.names.txt', 'w') as f:
            f.writelines(k + '\n' for k in names)
        return self.path


def read_avi(path):
    """(width, height, fps, [frame bytes in file order]) of a file MjpegWriter wrote (walks ``movi``; what merge_parts
    needs, not a general AVI reader)."""
    with open(path, 'rb') as f:
        d = f.read()
    if d[:4] != b'RIFF' or d[8:12] != b'AVI ':
        raise ValueError('%s: not a RIFF AVI' % path)
    frames, info, pos = [], None, 12
    while pos + 8 <= len(d):
        cc, size = d[pos:pos + 4], struct.unpack('<I', d[pos + 4:pos + 8])[0]
        if cc == b'LIST' and d[pos + 8:pos + 12] == b'hdrl':
            a = d.index(b'avih', pos) + 8
            us, _, _, _, _, _, _, _, w, h = struct.unpack('<10I', d[a:a + 40])
            info = (w, h, int(round(1e6 / us)))
        elif cc == b'LIST' and d[pos + 8:pos + 12] == b'movi':
            q, end = pos + 12, pos + 8 + size
            while q + 8 <= end:
                n = struct.unpack('<I', d[q + 4:q + 8])[0]
                if d[q:q + 4] == b'00dc':
                    frames.append(d[q + 8:q + 8 + n])
                q += 8 + n + (n & 1)
        pos += 8 + size + (size & 1)
    if info is None:
        raise ValueError('%s: no hdrl list' % path)
    return info + (frames,)


def merge_parts(paths, out_path):
    """The files ``paths`` (each with its ``.names.txt``: the per-rank parts of a frame-sharded run) as ONE file
    ``out_path`` with all their frames sorted by name: the chunks are copied, nothing is encoded again, and the result
    equals what one MjpegWriter given every frame writes.  Returns ``out_path``."""
    writer = None
    for p in paths:
        w, h, fps, frames = read_avi(p)
        with open(p + '.names.txt') as f:
            names = [line.rstrip('\n') for line in f if line.rstrip('\n')]
        if len(names) != len(frames):
            raise ValueError('%s: %d frames but %d names in its .names.txt' % (p, len(frames), len(names)))
        if writer is None:
            writer = MjpegWriter(out_path, w, h, fps)
        elif (writer.width, writer.height, writer.fps) != (w, h, fps):
            raise ValueError('%s: %dx%d at %d fps does not match the first part' % (p, w, h, fps))
        for k, fr in zip(names, frames):
            writer.add(k, fr)
    if writer is None:
        raise ValueError('merge_parts: no parts')
    return writer.finalize()
