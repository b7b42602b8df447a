// Baseline JPEG encoding of 8-bit RGB images (hnrf_video.h; humannerf_amd/video.py is the numpy twin that writes the same
// bytes).  Integer arithmetic only.  Three launches per image: one wave per MCU codes it into its fixed slot of the
// workspace, one block scans the lengths, one wave per MCU copies its slot and the marker behind it into the stream.
#include <initializer_list>
#include "hnrf_common.h"
#include "hnrf_block_scan.h"

namespace hnrf {
namespace {

// One MCU's slot, a derived worst case: 6 blocks x (DC: 9-bit code + 11 amplitude bits, plus 63 coefficients x (16-bit
// code + 10 amplitude bits)) = 9948 bits = 1244 bytes once padded to a byte, doubled because every byte may be an FF
// that is stuffed, rounded up to a multiple of 64 bytes.  (A coefficient costs at most 26 bits with or without the
// ZRL codes in front of it: a ZRL's 11 bits stand for 16 zeros that would cost nothing.)
constexpr int kSlot = HNRF_JPEG_SLOT_BYTES;
constexpr int kMcuBits = 6 * ((9 + 11) + 63 * (16 + 10));
constexpr int kMcuBytes = (kMcuBits + 7) / 8;
static_assert(kSlot == (2 * kMcuBytes + 63) / 64 * 64, "HNRF_JPEG_SLOT_BYTES is the derived bound");
// the LDS bit buffer in 32-bit words; a code of up to 59 bits at any bit offset touches three words
constexpr int kBufWords = (kMcuBytes + 3) / 4 + 3;
constexpr int kHeaderMax = 1024;

// ITU-T T.81 Annex K
constexpr uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                   14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                   18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// kZigzag[j] = the natural index of the j-th coefficient of the scan
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
    0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
    0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
    0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
    0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
    0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
    0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
    0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa};

// code and length per symbol (length 0: the symbol has no code), T.81 Annex C
struct Huff {
    uint16_t code[256];
    uint8_t len[256];
};
constexpr Huff make_huff(const uint8_t (&bits)[16], const uint8_t* vals) {
    Huff h{};
    unsigned c = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++c, ++k) {
            h.code[vals[k]] = (uint16_t)c;
            h.len[vals[k]] = (uint8_t)l;
        }
        c <<= 1;
    }
    return h;
}
struct Tables {
    Huff dc[2], ac[2];          // [0] luminance, [1] chrominance
    int dct[64];                // round(2^14 c_k cos((2n + 1) k pi / 16)), [k][n]
    uint8_t base[2][64];        // the Annex-K quantisation tables
    uint8_t zigpos[64];         // the scan position of natural index i
};
constexpr Tables make_tables() {
    Tables t{};
    t.dc[0] = make_huff(kDcLumaBits, kDcVals);
    t.dc[1] = make_huff(kDcChromaBits, kDcVals);
    t.ac[0] = make_huff(kAcLumaBits, kAcLumaVals);
    t.ac[1] = make_huff(kAcChromaBits, kAcChromaVals);
    constexpr int c[8][8] = {{5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793},
                             {8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035},
                             {7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568},
                             {6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811},
                             {5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793},
                             {4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551},
                             {3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135},
                             {1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598}};
    for (int i = 0; i < 64; ++i) {
        t.dct[i] = c[i >> 3][i & 7];
        t.base[0][i] = kBaseLuma[i];
        t.base[1][i] = kBaseChroma[i];
        t.zigpos[kZigzag[i]] = (uint8_t)i;
    }
    return t;
}
__constant__ const Tables kTab = make_tables();

__host__ __device__ inline int quality_scale(int q) { return q < 50 ? 5000 / q : 200 - 2 * q; }
__host__ __device__ inline int quant_entry(int base, int scale) {
    const int v = (base * scale + 50) / 100;
    return v < 1 ? 1 : (v > 255 ? 255 : v);
}

// `n` bits (1 .. 59) of `sym` at bit `p` of the buffer, most significant first; word w holds the bytes 4w .. 4w + 3 in
// that order.  OR is order-independent, so the lanes of a wave need no order among them.
__device__ __forceinline__ void put_bits(uint32_t* buf, int p, uint64_t sym, int n) {
    const int w = p >> 5, e = n + (p & 31);                            // e <= 90: three words
    const uint64_t hi = e <= 64 ? sym << (64 - e) : sym >> (e - 64);
    const uint32_t lo = e > 64 ? (uint32_t)(sym << (96 - e)) : 0u;
    atomicOr(&buf[w], (uint32_t)(hi >> 32));
    if ((uint32_t)hi) atomicOr(&buf[w + 1], (uint32_t)hi);
    if (lo) atomicOr(&buf[w + 2], lo);
}

__device__ __forceinline__ int size_category(int v) { return 32 - __clz(v < 0 ? -v : v); }     // 0 for v == 0

// One wave = one MCU.  slots [n_mcu][kSlot], lens [n_mcu].
__global__ __launch_bounds__(kWave) void jpeg_mcu_kernel(const uint8_t* __restrict__ rgb, int H, int W, int64_t stride,
                                                         int mcus_x, int scale, uint8_t* __restrict__ slots,
                                                         uint32_t* __restrict__ lens) {
    __shared__ int s_in[6 * 64], s_t[6 * 64], s_k[6 * 64], s_c[64];
    __shared__ uint32_t s_bits[kBufWords];
    const int lane = threadIdx.x;
    const int64_t mcu = blockIdx.x;
    const int my = (int)(mcu / mcus_x), mx = (int)(mcu % mcus_x);
    s_c[lane] = kTab.dct[lane];
    for (int i = lane; i < kBufWords; i += kWave) s_bits[i] = 0u;

    // colour: lane = one 2 x 2 quad of the MCU; pixels past the right / bottom edge repeat the edge
    {
        const int qy = lane >> 3, qx = lane & 7;
        int Rs = 0, Gs = 0, Bs = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int py = 2 * qy + (d >> 1), px = 2 * qx + (d & 1);
            const int y = min(my * 16 + py, H - 1), x = min(mx * 16 + px, W - 1);
            const uint8_t* p = rgb + (int64_t)y * stride + 3 * (int64_t)x;
            const int R = p[0], G = p[1], B = p[2];
            Rs += R;
            Gs += G;
            Bs += B;
            const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
            s_in[((py >> 3) * 2 + (px >> 3)) * 64 + (py & 7) * 8 + (px & 7)] = Y - 128;
        }
        const int cb = (-11058 * Rs - 21710 * Gs + 32768 * Bs + (128 << 18) + (1 << 17)) >> 18;
        const int cr = (32768 * Rs - 27439 * Gs - 5329 * Bs + (128 << 18) + (1 << 17)) >> 18;
        s_in[4 * 64 + lane] = min(max(cb, 0), 255) - 128;
        s_in[5 * 64 + lane] = min(max(cr, 0), 255) - 128;
    }
    __syncthreads();
    const int r8 = lane >> 3, c8 = lane & 7;
    // rows: t[y][u], lane = (y, u)
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        int acc = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += s_c[c8 * 8 + x] * s_in[b * 64 + r8 * 8 + x];
        s_t[b * 64 + lane] = (acc + (1 << 9)) >> 10;
    }
    __syncthreads();
    // columns: F[v][u], lane = (v, u); quantised and stored at its scan position
    {
        const int zp = kTab.zigpos[lane];
        const int ql = quant_entry(kTab.base[0][lane], scale), qc = quant_entry(kTab.base[1][lane], scale);
        const int lim = lane == 0 ? 1024 : 1023;
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            int acc = 0;
#pragma unroll
            for (int y = 0; y < 8; ++y) acc += s_c[r8 * 8 + y] * s_t[b * 64 + y * 8 + c8];
            const int F = (acc + (1 << 17)) >> 18;
            const int Q = b < 4 ? ql : qc;
            const int a = (2 * (F < 0 ? -F : F) + Q) / (2 * Q);
            s_k[b * 64 + zp] = F < 0 ? max(-a, -lim) : min(a, 1023);
        }
    }
    __syncthreads();

    // entropy coding: lane j holds coefficient j of the block
    int bitpos = 0, pred = 0;
    for (int b = 0; b < 6; ++b) {
        const int t = b >= 4;
        int v = s_k[b * 64 + lane];
        const int dc = __shfl(v, 0, kWave);
        if (lane == 0 && b >= 1 && b < 4) v -= pred;                   // Y01 from Y00, ...; Y00, Cb, Cr from 0
        pred = dc;
        const unsigned long long coded = __ballot(v != 0 || lane == 0);
        uint64_t sym = 0;
        int n = 0;
        const int cat = size_category(v);
        const uint32_t amp = (uint32_t)(v > 0 ? v : v + (1 << cat) - 1);
        if (lane == 0) {
            sym = ((uint64_t)kTab.dc[t].code[cat] << cat) | amp;
            n = kTab.dc[t].len[cat] + cat;
        } else if (v != 0) {
            const unsigned long long below = coded & ((1ull << lane) - 1ull);          // (bit 0 is set)
            const int run = lane - (63 - __clzll((long long)below)) - 1;
            const int zl = kTab.ac[t].len[0xF0];
            const uint64_t zc = kTab.ac[t].code[0xF0];
            for (int i = 0; i < (run >> 4); ++i) {                      // up to three ZRL
                sym = (sym << zl) | zc;
                n += zl;
            }
            const int s = ((run & 15) << 4) | cat;
            const int l = kTab.ac[t].len[s];
            sym = (((sym << l) | kTab.ac[t].code[s]) << cat) | amp;
            n += l + cat;
        } else if (lane == kWave - 1) {                                 // coefficient 63 is zero: EOB
            sym = kTab.ac[t].code[0];
            n = kTab.ac[t].len[0];
        }
        int incl = n;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int u = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += u;
        }
        if (n) put_bits(s_bits, bitpos + incl - n, sym, n);
        bitpos += __shfl(incl, kWave - 1, kWave);
    }
    const int nbytes = (bitpos + 7) >> 3, pad = nbytes * 8 - bitpos;
    if (lane == 0 && pad) put_bits(s_bits, bitpos, (1ull << pad) - 1ull, pad);
    __syncthreads();

    // byte stuffing: FF -> FF 00
    uint8_t* slot = slots + mcu * kSlot;
    int extra = 0;
    for (int base = 0; base < nbytes; base += kWave) {
        const int k = base + lane;
        const bool in = k < nbytes;
        const uint32_t byte = in ? (s_bits[k >> 2] >> (24 - 8 * (k & 3))) & 0xFFu : 0u;
        const bool ff = in && byte == 0xFFu;
        const unsigned long long bal = __ballot(ff);
        const int pos = k + extra + __popcll(bal & ((1ull << lane) - 1ull));
        if (in && pos + 1 < kSlot) {                                    // (always: 2 * kMcuBytes <= kSlot)
            slot[pos] = (uint8_t)byte;
            if (ff) slot[pos + 1] = 0;
        }
        extra += __popcll(bal);
    }
    if (lane == 0) lens[mcu] = (uint32_t)min(nbytes + extra, kSlot);
}

// offs[i] = the bytes of the MCUs before i with their two marker bytes each; offs[n] = all of them.  One block.
__global__ __launch_bounds__(kScanThreads) void jpeg_scan_kernel(const uint32_t* __restrict__ lens, int64_t n,
                                                                 uint32_t* __restrict__ offs) {
    uint32_t carry = 0;
    for (int64_t base = 0; base < n; base += kScanThreads) {
        const int64_t i = base + threadIdx.x;
        const int v = i < n ? (int)lens[i] + 2 : 0;
        int total;
        const int before = block_exclusive_scan(v, &total);
        if (i < n) offs[i] = carry + (uint32_t)before;
        carry += (uint32_t)total;
    }
    if (threadIdx.x == 0) offs[n] = carry;
}

// Block 0: the header and the length word; block 1 + m: MCU m and the marker behind it.
__global__ __launch_bounds__(kWave) void jpeg_gather_kernel(const uint8_t* __restrict__ header, int header_len,
                                                            const uint8_t* __restrict__ slots,
                                                            const uint32_t* __restrict__ lens,
                                                            const uint32_t* __restrict__ offs, int64_t n,
                                                            uint8_t* __restrict__ out, uint32_t* __restrict__ out_len) {
    const int lane = threadIdx.x;
    if (blockIdx.x == 0) {
        for (int i = lane; i < header_len; i += kWave) out[i] = header[i];
        if (lane == 0) *out_len = (uint32_t)header_len + offs[n];
        return;
    }
    const int64_t m = (int64_t)blockIdx.x - 1;
    const uint8_t* src = slots + m * kSlot;
    uint8_t* dst = out + header_len + offs[m];
    const int len = (int)lens[m];
    for (int i = lane; i < len; i += kWave) dst[i] = src[i];
    if (lane == 0) {
        dst[len] = 0xFF;
        dst[len + 1] = m + 1 < n ? (uint8_t)(0xD0 + (m & 7)) : (uint8_t)0xD9;
    }
}

inline bool size_ok(int H, int W) { return H >= 1 && W >= 1 && H <= 65535 && W <= 65535; }
inline int64_t mcu_count(int H, int W) { return (int64_t)((H + 15) / 16) * ((W + 15) / 16); }

}  // namespace
}  // namespace hnrf

using namespace hnrf;

extern "C" size_t hnrf_jpeg_workspace_bytes(int H, int W) {
    if (!size_ok(H, W)) return 0;
    const size_t n = (size_t)mcu_count(H, W);
    return align256(n * kSlot) + align256(n * 4) + align256((n + 1) * 4);       // slots | lens | offs
}

extern "C" size_t hnrf_jpeg_max_bytes(int H, int W) {
    if (!size_ok(H, W)) return 0;
    return (size_t)kHeaderMax + (size_t)mcu_count(H, W) * (kSlot + 2);
}

extern "C" int hnrf_jpeg_header(int H, int W, int quality, uint8_t* host_out, int cap) {
    HNRF_REQUIRE(size_ok(H, W), HNRF_E_ARG, "hnrf_jpeg_header: sizes are 1 .. 65535 per side, got H=%d W=%d", H, W);
    HNRF_REQUIRE(quality >= 1 && quality <= 100, HNRF_E_ARG, "hnrf_jpeg_header: quality %d (1 .. 100)", quality);
    HNRF_REQUIRE(host_out, HNRF_E_ARG, "hnrf_jpeg_header: null pointer");
    uint8_t h[kHeaderMax];
    int n = 0;
    auto put = [&](int v) { h[n++] = (uint8_t)v; };
    auto put16 = [&](int v) {
        put(v >> 8);
        put(v & 255);
    };
    put16(0xFFD8);
    put16(0xFFE0);                                                      // APP0: JFIF 1.1, no density, no thumbnail
    put16(16);
    for (int v : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) put(v);      // "JFIF\0" ...
    put16(0xFFDB);
    put16(2 + 65 + 65);
    const int scale = quality_scale(quality);
    for (int t = 0; t < 2; ++t) {
        put(t);
        for (int j = 0; j < 64; ++j) put(quant_entry(t ? kBaseChroma[kZigzag[j]] : kBaseLuma[kZigzag[j]], scale));
    }
    put16(0xFFC0);
    put16(17);
    put(8);
    put16(H);
    put16(W);
    for (int v : {3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1}) put(v);
    put16(0xFFC4);
    put16(2 + 2 * (17 + 12) + 2 * (17 + 162));
    auto dht = [&](int id, const uint8_t* bits, const uint8_t* vals, int nv) {
        put(id);
        for (int i = 0; i < 16; ++i) put(bits[i]);
        for (int i = 0; i < nv; ++i) put(vals[i]);
    };
    dht(0x00, kDcLumaBits, kDcVals, 12);
    dht(0x10, kAcLumaBits, kAcLumaVals, 162);
    dht(0x01, kDcChromaBits, kDcVals, 12);
    dht(0x11, kAcChromaBits, kAcChromaVals, 162);
    put16(0xFFDD);                                                      // DRI = 1
    put16(4);
    put16(1);
    put16(0xFFDA);
    put16(12);
    for (int v : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) put(v);
    HNRF_REQUIRE(cap >= n, HNRF_E_ARG, "hnrf_jpeg_header: room for %d bytes, %d needed", cap, n);
    for (int i = 0; i < n; ++i) host_out[i] = h[i];
    return n;
}

extern "C" int hnrf_jpeg_encode(const uint8_t* rgb, int H, int W, int64_t row_stride, const uint8_t* header, int header_len,
                                int quality, void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_cap,
                                uint32_t* out_len, void* stream) {
    HNRF_REQUIRE(size_ok(H, W), HNRF_E_ARG, "hnrf_jpeg_encode: sizes are 1 .. 65535 per side, got H=%d W=%d", H, W);
    HNRF_REQUIRE(quality >= 1 && quality <= 100, HNRF_E_ARG, "hnrf_jpeg_encode: quality %d (1 .. 100)", quality);
    HNRF_REQUIRE(rgb && header && workspace && out && out_len, HNRF_E_ARG, "hnrf_jpeg_encode: null pointer");
    HNRF_REQUIRE(row_stride >= 3 * (int64_t)W, HNRF_E_ARG, "hnrf_jpeg_encode: row_stride %lld below 3 W = %lld",
                 (long long)row_stride, 3 * (long long)W);
    HNRF_REQUIRE(header_len >= 1 && header_len <= kHeaderMax, HNRF_E_ARG, "hnrf_jpeg_encode: header_len %d (1 .. %d)",
                 header_len, kHeaderMax);
    HNRF_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)out_len & 3) == 0, HNRF_E_ARG,
                 "hnrf_jpeg_encode: workspace must be 256-byte aligned, out_len 4-byte aligned");
    const size_t max_bytes = hnrf_jpeg_max_bytes(H, W);
    HNRF_REQUIRE(max_bytes <= 0xFFFFFFFFull, HNRF_E_UNSUPPORTED,
                 "hnrf_jpeg_encode: %d x %d can take %zu bytes, more than the uint32 length word holds", H, W, max_bytes);
    const size_t need = hnrf_jpeg_workspace_bytes(H, W);
    HNRF_REQUIRE(workspace_bytes >= need, HNRF_E_WORKSPACE, "hnrf_jpeg_encode: workspace of %zu bytes, %zu needed",
                 workspace_bytes, need);
    HNRF_REQUIRE(out_cap >= max_bytes, HNRF_E_WORKSPACE, "hnrf_jpeg_encode: out_cap %zu below hnrf_jpeg_max_bytes = %zu",
                 out_cap, max_bytes);
    const int64_t n = mcu_count(H, W);
    uint8_t* slots = (uint8_t*)workspace;
    uint32_t* lens = (uint32_t*)(slots + align256((size_t)n * kSlot));
    uint32_t* offs = (uint32_t*)((uint8_t*)lens + align256((size_t)n * 4));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_mcu_kernel, dim3((unsigned)n), dim3(kWave), 0, st, rgb, H, W, row_stride, (W + 15) / 16,
                       quality_scale(quality), slots, lens);
    if (int rc = check_launch("hnrf_jpeg_encode (mcu)")) return rc;
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, (const uint32_t*)lens, n, offs);
    if (int rc = check_launch("hnrf_jpeg_encode (scan)")) return rc;
    hipLaunchKernelGGL(jpeg_gather_kernel, dim3((unsigned)(n + 1)), dim3(kWave), 0, st, header, header_len,
                       (const uint8_t*)slots, (const uint32_t*)lens, (const uint32_t*)offs, n, out, out_len);
    return check_launch("hnrf_jpeg_encode (gather)");
}
