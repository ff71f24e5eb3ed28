// Baseline JPEG encoder (ITU T.81, JFIF, 8-bit YCbCr 4:2:0) over a batch of uint8 HWC frames: the stream
// contract of include/s2v.h (s2v_jpeg_encode), all in integers, so the bytes are reproducible.
//
//   1. jpeg_transform: one wave per 16x16 MCU.  The patch (edge-replicated past the frame) is converted to
//      Y / Cb / Cr in LDS, chroma is summed 2x2, and lane (u, c) does the two integer matrix passes of the six
//      8x8 blocks, T = (CI X + 1024) >> 11 and F = (T CI^T + 16384) >> 15, then quantises.  int16 coefficients
//      in zigzag order go to the workspace as [n][mcu][6][64].
//   2. jpeg_entropy: one workgroup per (frame, MCU row) = restart interval, in tiles of 32 MCUs (192 blocks:
//      a block's longest code is 1658 bits, kept as 52 words of LDS).  Each lane takes a block: a first
//      pass counts its bits, a workgroup scan gives its bit offset, a second pass ORs the bits into zeroed LDS
//      words (OR commutes: deterministic).  The tile's whole bytes are then stuffed (0xFF -> 0xFF 0x00) with
//      a scan over the 0xFF count and stored to the interval's staging area; the 0-7 bits left over lead the
//      next tile.  The last byte of the interval is padded with 1-bits.
//   3. jpeg_compact: one workgroup per (frame, MCU row).  It sums the interval sizes of the frame (its own
//      offset and the file size), and copies its interval and the marker after it (RSTm, or EOI after the last
//      row; row 0 also the header) into the frame's slot, unless the file does not fit.
#include "common.hpp"

namespace s2v {
namespace {

constexpr int JT_THREADS = 256;            // transform: 4 waves, one MCU each
constexpr int JE_THREADS = 256;
constexpr int JE_TILE_MCUS = 32;
constexpr int JE_TILE_BLOCKS = JE_TILE_MCUS * 6;
constexpr int JE_BLOCK_WORDS = 52;         // 1664 bits >= 20 (DC) + 63 * 26 (AC) = 1658
constexpr int JE_WORDS = JE_TILE_BLOCKS * JE_BLOCK_WORDS + 2;
constexpr int JE_BLOCK_BYTES = 2 * 4 * JE_BLOCK_WORDS;   // a block's stuffed worst case: 416 bytes

// CI[u][x] = rint(8192 k(u) cos((2x + 1) u pi / 16)), k(0) = sqrt(1/8), k(u > 0) = 1/2
__constant__ int c_ci[64] = {
    2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,
    4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,
    3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,
    3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,
    2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,
    2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,
    1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,
    799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};

// zigzag position of natural index u * 8 + v
__constant__ unsigned char c_zz_of_nat[64] = {
    0,  1,  5,  6,  14, 15, 27, 28,
    2,  4,  7,  13, 16, 26, 29, 42,
    3,  8,  12, 17, 25, 30, 41, 43,
    9,  11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54,
    20, 22, 33, 38, 46, 51, 55, 60,
    21, 34, 37, 47, 50, 56, 59, 61,
    35, 36, 48, 49, 57, 58, 62, 63};

// T.81 Annex K.3 typical Huffman tables: BITS (codes per length 1..16) and HUFFVAL
struct HuffSpec {
    unsigned char bits[16];
    unsigned char vals[162];
};
constexpr HuffSpec K3_DC0 = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec K3_DC1 = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec K3_AC0 = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec K3_AC1 = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// code tables by symbol (T.81 Annex C): entry = code << 8 | length, 0 for a symbol without a code;
// [0] DC luma, [1] DC chroma, [2] AC luma, [3] AC chroma
struct HuffTabs {
    unsigned e[4][256];
};

constexpr void huff_fill(unsigned (&e)[256], const HuffSpec &s) {
    for (int i = 0; i < 256; ++i) e[i] = 0u;
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) e[s.vals[k++]] = (code++ << 8) | (unsigned)len;
        code <<= 1;
    }
}

constexpr HuffTabs huff_tabs() {
    HuffTabs t{};
    huff_fill(t.e[0], K3_DC0);
    huff_fill(t.e[1], K3_DC1);
    huff_fill(t.e[2], K3_AC0);
    huff_fill(t.e[3], K3_AC1);
    return t;
}

__constant__ HuffTabs c_huff = huff_tabs();

struct JpegDims {
    int mcols, mrows, mcus;        // MCUs per row, MCU rows, MCUs per frame
    long coef_bytes, sizes_bytes;  // workspace parts (multiples of 16), all frames
    long row_stage;                // staging bytes per interval (a multiple of 16)
    long total;
};

inline JpegDims jpeg_dims(int n, int h, int w) {
    JpegDims d;
    d.mcols = (w + 15) / 16;
    d.mrows = (h + 15) / 16;
    d.mcus = d.mcols * d.mrows;
    d.coef_bytes = (long)n * d.mcus * 6 * 64 * 2;
    d.sizes_bytes = (((long)n * d.mrows * 4) + 15) & ~15L;
    d.row_stage = (long)d.mcols * 6 * JE_BLOCK_BYTES;
    d.total = d.coef_bytes + d.sizes_bytes + (long)n * d.mrows * d.row_stage + 16;   // + 16: the copy reads whole words
    return d;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(JT_THREADS) void jpeg_transform(const unsigned char *__restrict__ frames, int h, int w,
                                                             long pitch, long frame_stride, int bgr, int mcols,
                                                             int mcus, const unsigned short *__restrict__ qt,
                                                             short *__restrict__ coef) {
    __shared__ int s_full[4][3][256];      // Y - 128, Cb, Cr of the 16x16 patch
    __shared__ int s_chroma[4][2][64];     // 2x2 sums - 128
    __shared__ int s_t[4][6][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    const int mcu_raw = blockIdx.x * 4 + wave;
    const bool live = mcu_raw < mcus;
    const int mcu = live ? mcu_raw : mcus - 1;
    const int my = mcu / mcols, mx = mcu - my * mcols;
    const unsigned char *img = frames + (long)b * frame_stride;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = lane + 64 * i, py = p >> 4, px = p & 15;
        int gy = my * 16 + py, gx = mx * 16 + px;
        gy = gy < h ? gy : h - 1;
        gx = gx < w ? gx : w - 1;
        const unsigned char *q = img + (long)gy * pitch + (long)gx * 3;
        const int c0 = q[0], c1 = q[1], c2 = q[2];
        const int R = bgr ? c2 : c0, G = c1, B = bgr ? c0 : c2;
        s_full[wave][0][p] = clamp255((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
        s_full[wave][1][p] = clamp255((-11059 * R - 21709 * G + 32768 * B + 32768 + (128 << 16)) >> 16);
        s_full[wave][2][p] = clamp255((32768 * R - 27439 * G - 5329 * B + 32768 + (128 << 16)) >> 16);
    }
    __syncthreads();
    {
        const int cy = lane >> 3, cx = lane & 7, p = (2 * cy) * 16 + 2 * cx;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int *f = s_full[wave][1 + c];
            s_chroma[wave][c][lane] = ((f[p] + f[p + 1] + f[p + 16] + f[p + 17] + 2) >> 2) - 128;
        }
    }
    __syncthreads();
    const int u = lane >> 3, v = lane & 7;   // pass 1: T[u][c = v]; pass 2: F[u][v]
    int ciu[8], civ[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        ciu[i] = c_ci[u * 8 + i];
        civ[i] = c_ci[v * 8 + i];
    }
#pragma unroll
    for (int blk = 0; blk < 6; ++blk) {
        int acc = 1024;
        if (blk < 4) {
            const int *X = s_full[wave][0] + (blk >> 1) * 128 + (blk & 1) * 8;   // rows of 16
#pragma unroll
            for (int r = 0; r < 8; ++r) acc += ciu[r] * X[r * 16 + v];
        } else {
            const int *X = s_chroma[wave][blk - 4];
#pragma unroll
            for (int r = 0; r < 8; ++r) acc += ciu[r] * X[r * 8 + v];
        }
        s_t[wave][blk][lane] = acc >> 11;
    }
    __syncthreads();
    const int z = c_zz_of_nat[lane];
    short *dst = coef + ((long)b * mcus + mcu) * 6 * 64;
#pragma unroll
    for (int blk = 0; blk < 6; ++blk) {
        int acc = 16384;
        const int *T = s_t[wave][blk] + u * 8;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc += T[c] * civ[c];
        const int F = acc >> 15;
        const int t = qt[(blk < 4 ? 0 : 64) + z];
        int q = ((F < 0 ? -F : F) + (t >> 1)) / t;
        q = F < 0 ? -q : q;
        if (z == 0) q = q < -1024 ? -1024 : (q > 1023 ? 1023 : q);
        else q = q < -1023 ? -1023 : (q > 1023 ? 1023 : q);
        if (live) dst[blk * 64 + z] = (short)q;
    }
}

// exclusive scan of v over the workgroup (JE_THREADS = 4 waves); total: the sum, in every thread
__device__ __forceinline__ int block_exclusive_scan(int v, int *s_wave, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                       // s_wave of the previous scan has been read
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int i = 0; i < JE_THREADS / 64; ++i) {
        const int t = s_wave[i];
        before += i < wave ? t : 0;
        sum += t;
    }
    total = sum;
    return before + inc - v;
}

struct BitCount {
    int n = 0;
    __device__ __forceinline__ void put(unsigned, int len) { n += len; }
};

// ORs (code, len <= 26) at a running bit position into big-endian words of LDS: bit 31 of a word comes first
struct BitWrite {
    unsigned *words;
    int pos;
    unsigned acc = 0;
    __device__ __forceinline__ void put(unsigned code, int len) {
        const int off = pos & 31;
        const unsigned long long v = (unsigned long long)code << (64 - off - len);
        acc |= (unsigned)(v >> 32);
        if (off + len >= 32) {
            const int wi = pos >> 5;
            if (wi < JE_WORDS) atomicOr(&words[wi], acc);
            acc = (unsigned)v;
        }
        pos += len;
    }
    __device__ __forceinline__ void flush() {
        const int wi = pos >> 5;
        if (acc && wi < JE_WORDS) atomicOr(&words[wi], acc);
    }
};

// T.81 F.1.2 of one block: blk[64] zigzag coefficients, pred the DC predictor, dc / ac its code tables
template <class Sink>
__device__ __forceinline__ void jpeg_block(const short *__restrict__ blk, int pred, const unsigned *dc,
                                           const unsigned *ac, Sink &sink) {
    int run = 0;
    for (int q = 0; q < 8; ++q) {
        const uint4 raw = ((const uint4 *)blk)[q];
        const unsigned r[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int c = (short)((r[i >> 1] >> (16 * (i & 1))) & 0xffffu);
            const bool is_dc = q == 0 && i == 0;
            if (is_dc) c -= pred;
            if (c == 0 && !is_dc) {
                ++run;
                continue;
            }
            const int a = c < 0 ? -c : c;
            const int cat = a ? 32 - __clz(a) : 0;
            const unsigned extra = (unsigned)(c < 0 ? c - 1 : c) & ((1u << cat) - 1u);
            unsigned e;
            if (is_dc) {
                e = dc[cat];
            } else {
                const unsigned zrl = ac[0xf0];
                while (run >= 16) {
                    sink.put(zrl >> 8, (int)(zrl & 255u));
                    run -= 16;
                }
                e = ac[(run << 4) | cat];
                run = 0;
            }
            const int len = (int)(e & 255u);
            sink.put(((e >> 8) << cat) | extra, len + cat);
        }
    }
    if (run > 0) {
        const unsigned eob = ac[0];
        sink.put(eob >> 8, (int)(eob & 255u));
    }
}

__global__ __launch_bounds__(JE_THREADS) void jpeg_entropy(const short *__restrict__ coef, int mcols, int mrows,
                                                           int mcus, unsigned char *__restrict__ stage,
                                                           long row_stage, int *__restrict__ row_bytes) {
    __shared__ unsigned s_bits[JE_WORDS];
    __shared__ unsigned s_huff[4][256];
    __shared__ int s_wave[JE_THREADS / 64];
    const int tid = threadIdx.x;
    const int row = blockIdx.x, b = blockIdx.y;
    for (int i = tid; i < 4 * 256; i += JE_THREADS) s_huff[i >> 8][i & 255] = c_huff.e[i >> 8][i & 255];
    const short *rowc = coef + ((long)b * mcus + (long)row * mcols) * 6 * 64;
    unsigned char *dst = stage + ((long)b * mrows + row) * row_stage;
    long outpos = 0;
    int carry_n = 0;
    unsigned carry_v = 0;                  // the carry_n bits left of the previous tile
    for (int m0 = 0; m0 < mcols; m0 += JE_TILE_MCUS) {
        const int tile_mcus = mcols - m0 < JE_TILE_MCUS ? mcols - m0 : JE_TILE_MCUS;
        const bool last = m0 + tile_mcus == mcols;
        const bool active = tid < tile_mcus * 6;
        const int m = m0 + tid / 6, j = tid % 6;
        const short *blk = rowc + ((long)m * 6 + j) * 64;
        int pred = 0;
        if (active) {
            if (j >= 1 && j <= 3) pred = blk[-64];
            else if (m > 0) pred = j == 0 ? blk[-3 * 64] : blk[-6 * 64];
        }
        const unsigned *dc = s_huff[j < 4 ? 0 : 1], *ac = s_huff[j < 4 ? 2 : 3];
        __syncthreads();                   // s_huff is filled; the previous tile's s_bits have been read
        int nbits = 0;
        if (active) {
            BitCount cnt;
            jpeg_block(blk, pred, dc, ac, cnt);
            nbits = cnt.n;
        }
        int tile_bits;
        const int at = block_exclusive_scan(nbits, s_wave, tile_bits);
        int tot = carry_n + tile_bits;
        const int nwords = (tot >> 5) + 2;  // <= JE_WORDS
        for (int i = tid; i < nwords; i += JE_THREADS) s_bits[i] = (i == 0 && carry_n) ? carry_v << (32 - carry_n) : 0u;
        __syncthreads();
        if (active) {
            BitWrite wr{s_bits, carry_n + at};
            jpeg_block(blk, pred, dc, ac, wr);
            wr.flush();
        }
        __syncthreads();
        if (last && (tot & 7)) {
            const int pad = 8 - (tot & 7);
            if (tid == 0) s_bits[tot >> 5] |= ((1u << pad) - 1u) << (32 - (tot & 31) - pad);
            tot += pad;
            __syncthreads();
        }
        const int nbytes = tot >> 3;
        carry_n = tot & 7;
        carry_v = carry_n ? ((s_bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u) >> (8 - carry_n) : 0u;
        // ---- stuff and store the tile's whole bytes: a word (4 stream bytes) per thread and step
        for (int base = 0; base < nbytes; base += 4 * JE_THREADS) {
            const int i0 = base + 4 * tid;
            const unsigned wv = i0 < nbytes ? s_bits[i0 >> 2] : 0u;
            const int valid = nbytes - i0 < 4 ? (nbytes - i0 < 0 ? 0 : nbytes - i0) : 4;
            int ff = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) ff += (k < valid && ((wv >> (24 - 8 * k)) & 255u) == 255u) ? 1 : 0;
            int ff_total;
            const int ff_before = block_exclusive_scan(ff, s_wave, ff_total);
            long o = outpos + 4 * tid + ff_before;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < valid) {
                    const unsigned byte = (wv >> (24 - 8 * k)) & 255u;
                    if (o < row_stage) dst[o] = (unsigned char)byte;
                    ++o;
                    if (byte == 255u) {
                        if (o < row_stage) dst[o] = 0;
                        ++o;
                    }
                }
            }
            const int step = nbytes - base < 4 * JE_THREADS ? nbytes - base : 4 * JE_THREADS;
            outpos += step + ff_total;
        }
    }
    if (tid == 0) row_bytes[(long)b * mrows + row] = (int)outpos;
}

__global__ __launch_bounds__(256) void jpeg_compact(const unsigned char *__restrict__ stage, long row_stage,
                                                    const int *__restrict__ row_bytes, int mrows,
                                                    const unsigned char *__restrict__ header, int header_bytes,
                                                    unsigned char *__restrict__ out, long capacity,
                                                    int *__restrict__ sizes, int *__restrict__ status) {
    __shared__ long s_red[2][256];
    const int tid = threadIdx.x, row = blockIdx.x, b = blockIdx.y;
    const int *rb = row_bytes + (long)b * mrows;
    long before = 0, all = 0;
    for (int i = tid; i < mrows; i += 256) {
        const long v = rb[i];
        all += v;
        before += i < row ? v : 0;
    }
    s_red[0][tid] = before;
    s_red[1][tid] = all;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) {
            s_red[0][tid] += s_red[0][tid + d];
            s_red[1][tid] += s_red[1][tid + d];
        }
        __syncthreads();
    }
    // every interval is followed by a two-byte marker: RSTm, or EOI after the last
    const long total = (long)header_bytes + s_red[1][0] + 2L * mrows;
    const long off = (long)header_bytes + s_red[0][0] + 2L * row;
    const bool fits = total <= capacity;
    if (row == 0 && tid == 0) {
        sizes[b] = (int)total;
        status[b] = fits ? 0 : 1;
    }
    if (!fits) return;
    unsigned char *slot = out + (long)b * capacity;
    if (row == 0)
        for (int i = tid; i < header_bytes; i += 256) slot[i] = header[i];
    const long len = rb[row];
    const unsigned char *src = stage + ((long)b * mrows + row) * row_stage;   // 16-byte aligned
    unsigned char *dst = slot + off;
    long head = (long)((4u - (unsigned)((size_t)dst & 3u)) & 3u);
    head = head < len ? head : len;
    if (tid < head) dst[tid] = src[tid];
    const long nw = (len - head) >> 2;
    const unsigned *src32 = (const unsigned *)src;
    unsigned *dst32 = (unsigned *)(dst + head);
    const unsigned sh = (unsigned)(head & 3) * 8u;
    for (long i = tid; i < nw; i += 256) {
        const long s = (head >> 2) + i;                                      // head < 4: words s and s + 1
        const unsigned lo = src32[s], hi = src32[s + 1];
        dst32[i] = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
    }
    const long done = head + 4 * nw;
    if (tid < len - done) dst[done + tid] = src[done + tid];
    if (tid == 0) {
        dst[len] = 0xff;
        dst[len + 1] = row + 1 < mrows ? (unsigned char)(0xd0 + (row & 7)) : (unsigned char)0xd9;
    }
}

}  // namespace
}  // namespace s2v

using namespace s2v;

extern "C" long s2v_jpeg_ws_bytes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535) return 0;
    return jpeg_dims(n, h, w).total;
}

extern "C" long s2v_jpeg_worst_bytes(int h, int w) {
    if (h <= 0 || w <= 0 || h > 65535 || w > 65535) return 0;
    const JpegDims d = jpeg_dims(1, h, w);
    return (long)d.mrows * (d.row_stage + 2);
}

extern "C" int s2v_jpeg_encode(const uint8_t *frames, int n, int h, int w, long pitch_bytes, long frame_stride_bytes,
                               int bgr, const uint8_t *header, int header_bytes, const uint16_t *qtables, uint8_t *out,
                               long capacity, int *sizes, int *status, void *ws, long ws_bytes, s2v_stream_t stream) {
    S2V_REQUIRE(frames && header && qtables && out && sizes && status && ws, "jpeg_encode: null pointer");
    S2V_REQUIRE(n > 0 && n <= 65535 && h > 0 && w > 0 && h <= 65535 && w <= 65535, "jpeg_encode: n %d, h %d, w %d", n,
                h, w);
    S2V_REQUIRE(pitch_bytes >= 3L * w && frame_stride_bytes >= 0, "jpeg_encode: pitch %ld (>= 3 w), frame stride %ld",
                pitch_bytes, frame_stride_bytes);
    S2V_REQUIRE(bgr == 0 || bgr == 1, "jpeg_encode: bgr %d (0 or 1)", bgr);
    S2V_REQUIRE(header_bytes > 0 && capacity > 0, "jpeg_encode: header_bytes %d, capacity %ld", header_bytes, capacity);
    const JpegDims d = jpeg_dims(n, h, w);
    S2V_REQUIRE((long)header_bytes + (long)d.mrows * (d.row_stage + 2) < (1L << 31), "jpeg_encode: frame too large");
    S2V_REQUIRE(ws_bytes >= d.total && ((size_t)ws & 15) == 0, "jpeg_encode: workspace %ld bytes (need %ld, 16-byte aligned)",
                ws_bytes, d.total);
    short *coef = (short *)ws;
    int *row_bytes = (int *)((char *)ws + d.coef_bytes);
    unsigned char *stage = (unsigned char *)ws + d.coef_bytes + d.sizes_bytes;
    hipStream_t st = (hipStream_t)stream;
    jpeg_transform<<<dim3(cdiv(d.mcus, 4), n), JT_THREADS, 0, st>>>(frames, h, w, pitch_bytes, frame_stride_bytes, bgr,
                                                                    d.mcols, d.mcus, qtables, coef);
    jpeg_entropy<<<dim3(d.mrows, n), JE_THREADS, 0, st>>>(coef, d.mcols, d.mrows, d.mcus, stage, d.row_stage, row_bytes);
    jpeg_compact<<<dim3(d.mrows, n), 256, 0, st>>>(stage, d.row_stage, row_bytes, d.mrows, header, header_bytes, out,
                                                   capacity, sizes, status);
    return check_launch("jpeg_encode");
}
