// The arithmetic of the baseline JPEG decoder (s2v_jpeg_decode, include/s2v.h), written once for the device
// kernels (jpeg_dec.hip) and for the stand-alone host program (tools/jpeg_decode_host.cpp): the T.81 F.2.2
// entropy decoder of one restart interval, jidctint's 1-D ISLOW pass, libjpeg's fancy chroma upsampling and the
// YCbCr -> RGB conversion.  Plain C++: no HIP header is needed to compile it for the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define S2V_JD __host__ __device__ __forceinline__
#else
#define S2V_JD inline
#endif

namespace s2v {
namespace jdec {

// A Huffman table as a DHT segment gives it: BITS[16] then HUFFVAL[256] (unused entries 0).  A set holds the six
// tables of one frame in the order (DC, AC) of component 0, (DC, AC) of component 1, (DC, AC) of component 2.
constexpr int HUFF_SPEC_BYTES = 16 + 256;
constexpr int HUFF_SET_TABLES = 6;
constexpr int HUFF_SET_BYTES = HUFF_SET_TABLES * HUFF_SPEC_BYTES;
constexpr int INTERVAL_INTS = 5;           // (byte offset, byte length, frame, first MCU, MCU count)

enum Status { ST_OK = 0, ST_BAD_CODE = 1, ST_RUN_PAST_63 = 2, ST_DATA_ENDS = 3, ST_BAD_TABLE = 4 };

// T.81 F.2.2.3: maxcode[l] is the largest code of length l (-1: none), valoff[l] = valptr[l] - mincode[l];
// look[v] = length << 8 | symbol for the code of at most 8 bits that leads the 8 bits v, 0 when it is longer
struct HuffTable {
    int maxcode[17];
    int valoff[17];
    unsigned short look[256];
    unsigned char huffval[256];
};

S2V_JD void huff_derive_codes(const unsigned char *spec, HuffTable &t) {
    int code = 0, k = 0;
    t.maxcode[0] = -1;
    t.valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int nb = spec[l - 1];
        t.valoff[l] = k - code;
        t.maxcode[l] = nb ? code + nb - 1 : -1;
        code = (code + nb) << 1;
        k += nb;
    }
}

// entry i of look and of huffval, once huff_derive_codes has run: the work of one of 256 lanes
S2V_JD void huff_derive_entry(const unsigned char *spec, HuffTable &t, int i) {
    t.huffval[i] = spec[16 + i];
    unsigned short e = 0;
    for (int l = 1; l <= 8; ++l) {
        const int code = i >> (8 - l);
        if (code <= t.maxcode[l]) {
            e = (unsigned short)((l << 8) | spec[16 + ((t.valoff[l] + code) & 255)]);
            break;
        }
    }
    t.look[i] = e;
}

// The bytes [pos, end) of one restart interval as a bit stream, 0xFF 0x00 unstuffed.  No byte at or past ``end`` is
// read: past the data the reader feeds zero bits and counts them in ``fake``; they sit below the true bits, so
// nbits < fake says that some were consumed.  A 0xFF followed by anything but 0x00 ends the data.
struct BitReader {
    const unsigned char *p;
    long pos, end;
    unsigned long long acc;
    int nbits, fake;

    S2V_JD void open(const unsigned char *base, long begin, long stop) {
        p = base;
        pos = begin;
        end = stop;
        acc = 0;
        nbits = 0;
        fake = 0;
    }
    // Bytes are read one at a time: reading eight aligned bytes per load was measured and changed nothing (the
    // serial decoder is bound by its own dependent instructions, not by the loads).
    S2V_JD void fill() {                   // afterwards nbits >= 57: a code (16) and its extra bits (15)
        while (nbits <= 56) {
            unsigned b = 0;
            if (pos < end) {
                b = p[pos++];
                if (b == 0xFFu) {
                    if (pos < end && p[pos] == 0) {
                        ++pos;
                    } else {
                        pos = end;         // a marker, or 0xFF as the last byte: the data ends
                        b = 0;
                        fake += 8;
                    }
                }
            } else {
                fake += 8;
            }
            acc = (acc << 8) | b;
            nbits += 8;
        }
    }
    S2V_JD unsigned peek(int n) const { return (unsigned)(acc >> (nbits - n)) & ((1u << n) - 1u); }
    S2V_JD void skip(int n) { nbits -= n; }
    S2V_JD bool ran_dry() const { return nbits < fake; }
};

// one symbol (call fill() first); -1: no code of up to 16 bits leads the stream.  Reader: BitReader or PosReader
template <class Reader>
S2V_JD int huff_decode(Reader &br, const HuffTable &t) {
    const unsigned v = br.peek(16);
    const unsigned e = t.look[v >> 8];
    if (e) {
        br.skip((int)(e >> 8));
        return (int)(e & 255u);
    }
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)(v >> (16 - l));
        if (code <= t.maxcode[l]) {
            br.skip(l);
            return t.huffval[(t.valoff[l] + code) & 255];
        }
    }
    return -1;
}

// T.81 F.2.2.1 EXTEND of the s-bit value v
S2V_JD int huff_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One 8x8 block (T.81 F.2.2): dst[64] int16 in zigzag order, all zero on entry; only non-zero positions and the
// DC are written.  pred: the component's DC predictor.  -> a Status.
S2V_JD int decode_block(BitReader &br, const HuffTable &dc, const HuffTable &ac, int &pred, short *dst) {
    br.fill();
    int s = huff_decode(br, dc);
    if (s < 0 || s > 11) return ST_BAD_CODE;
    if (s) {
        pred += huff_extend((int)br.peek(s), s);
        br.skip(s);
    }
    dst[0] = (short)pred;
    for (int k = 1; k < 64;) {
        br.fill();
        const int rs = huff_decode(br, ac);
        if (rs < 0) return ST_BAD_CODE;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;            // EOB
            k += 16;                       // ZRL: a coefficient must follow
            if (k > 63) return ST_RUN_PAST_63;
            continue;
        }
        k += r;
        if (k > 63) return ST_RUN_PAST_63;
        dst[k] = (short)huff_extend((int)br.peek(s), s);
        br.skip(s);
        ++k;
    }
    return br.ran_dry() ? ST_DATA_ENDS : ST_OK;
}

// component of block j of an MCU with hs x vs luma blocks: the luma blocks come first, then Cb, then Cr
S2V_JD int block_component(int j, int hs, int vs) { return j < hs * vs ? 0 : j - hs * vs + 1; }

// what the entropy decoder is given (s2v_jpeg_decode); none of the tables has been checked by the host
struct EntropyArgs {
    const unsigned char *stream;
    long stream_bytes;
    const int *intervals;          // [n_intervals][INTERVAL_INTS]
    int n_intervals;
    const int *frame_first;        // [n + 1]: frame b's intervals are frame_first[b] .. frame_first[b + 1] - 1
    int n, mcus, hs, vs, bpm;
    const unsigned char *huff_sets;
    int n_sets;
    const int *set_index;          // [n]
    short *coef;                   // [n][mcus][bpm][64], zigzag order
    int *status;                   // [n]
};

struct Interval {
    long off, end;
    int frame, first, count;
    bool ok;                       // every field lies inside the stream, the batch and the frame
};

S2V_JD Interval load_interval(const EntropyArgs &a, int iv) {
    const int *t = a.intervals + (long)iv * INTERVAL_INTS;
    Interval r;
    r.off = t[0];
    r.end = r.off + t[1];
    r.frame = t[2];
    r.first = t[3];
    r.count = t[4];
    r.ok = t[0] >= 0 && t[1] >= 0 && r.end <= a.stream_bytes && r.frame >= 0 && r.frame < a.n && r.first >= 0 &&
           r.count >= 0 && (long)r.first + r.count <= a.mcus;
    return r;
}

// A whole interval by one thread, straight into coefficients that are zero on entry -> a Status.  tab: the six
// derived tables of the frame's set.
S2V_JD int decode_interval(const EntropyArgs &a, const Interval &iv, const HuffTable *tab) {
    BitReader br;
    br.open(a.stream, iv.off, iv.end);
    int p0 = 0, p1 = 0, p2 = 0;
    short *dst = a.coef + ((long)iv.frame * a.mcus + iv.first) * a.bpm * 64;
    const int blocks = iv.count * a.bpm;
    int j = 0;
    for (int k = 0; k < blocks; ++k) {
        const int c = block_component(j, a.hs, a.vs);
        int &pred = c == 0 ? p0 : (c == 1 ? p1 : p2);
        const int err = decode_block(br, tab[2 * c], tab[2 * c + 1], pred, dst + (long)k * 64);
        if (err != ST_OK) return err;
        j = j + 1 == a.bpm ? 0 : j + 1;
    }
    return ST_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// The "sync" entropy decoder (s2v_jpeg_decode_sync): an interval is cut into subsequences of sub_bytes raw
// (stuffed) bytes, the last one shorter, and subsequence b is decoded from the state its left neighbour hands it.
//
// A state is (pos, j, k): pos the position of the next unread bit, 8 * (byte index in the stream) + bit, j the
// block within the MCU, k the zigzag index (0: a DC code comes next); packed pos << 16 | j << 8 | k.  Positions are
// canonical: once the last bit of a data byte 0xFF is consumed the position is that of the byte after its stuffed
// 0x00, and a state that points at a stuffed 0x00 is moved past it when it is opened.  Past the interval's end (or
// past a marker inside it) the reader feeds zero bits, as BitReader does, and the position goes on counting them.
constexpr int SYNC_SUB_MIN = 4, SYNC_SUB_MAX = 4096;
constexpr int SYNC_RECORD_BYTES = 48;      // per subsequence: two state buffers, the last entry state, a summary

S2V_JD unsigned long long sync_pack(long pos, int j, int k) {
    return ((unsigned long long)pos << 16) | ((unsigned)j << 8) | (unsigned)k;
}

// what one subsequence, decoded from its entry state, adds to the interval
struct SyncSummary {
    int blocks;                    // blocks closed
    int dc[3];                     // sum of the DC differences per component
    int err, err_block;            // the first Status that is not ST_OK and the (local) block it lies in
};

// BitReader that knows where it is.  smask bit i: byte i of acc, counted from the low end, is a 0xFF whose stuffed
// 0x00 was skipped; vpos: the next byte to load, counting on past the end of the data.
struct PosReader {
    const unsigned char *p;
    long vpos, end;
    unsigned long long acc;
    int nbits, fake;
    unsigned smask;
    bool dead;

    S2V_JD void open(const unsigned char *base, long off, long stop, long bitpos) {
        p = base;
        end = stop;
        acc = 0;
        nbits = 0;
        fake = 0;
        smask = 0;
        long b = bitpos >> 3;
        const int bit = (int)(bitpos & 7);
        dead = b >= end;
        if (!dead && bit == 0 && b > off && p[b - 1] == 0xFFu && p[b] == 0) ++b;   // a start on a stuffed 0x00
        vpos = b;
        fill();
        skip(bit);
    }
    S2V_JD void fill() {
        while (nbits <= 56) {
            unsigned b = 0, st = 0;
            if (!dead && vpos < end) {
                b = p[vpos];
                if (b == 0xFFu) {
                    if (vpos + 1 < end && p[vpos + 1] == 0) {
                        st = 1;
                        ++vpos;
                    } else {
                        dead = true;       // a marker, or 0xFF as the last byte: the data ends
                        b = 0;
                    }
                }
            } else {
                dead = true;
            }
            if (dead) fake += 8;
            ++vpos;
            acc = (acc << 8) | b;
            smask = (smask << 1) | st;
            nbits += 8;
        }
    }
    S2V_JD unsigned peek(int n) const { return (unsigned)(acc >> (nbits - n)) & ((1u << n) - 1u); }
    S2V_JD void skip(int n) { nbits -= n; }
    S2V_JD bool ran_dry() const { return nbits < fake; }
    // of the next unread bit, not of the read-ahead: a 0xFF with unread bits still has its 0x00 ahead of it
    S2V_JD long position() const {
        const int bytes = (nbits + 7) >> 3;
        const int ahead = __builtin_popcount(smask & ((1u << bytes) - 1u));
        return vpos * 8 - nbits - 8 * ahead;
    }
};

// F: subsequence [sub_begin, sub_end) of the interval [off, end), entered in ``state`` -> the exit state.  Symbols
// (a code and its extra bits) are decoded while the next one starts before sub_end; an entry position at or past
// sub_end passes through unchanged.  F is total, and what is an error to the serial decoder is only noted in
// ``sum`` and decoding goes on by a fixed rule:
//   no code leads the 16 bits (ST_BAD_CODE)     one bit is skipped, j and k stay;
//   a DC category above 11 (ST_BAD_CODE)        the code is consumed, the difference is 0, k = 1;
//   a run past coefficient 63 (ST_RUN_PAST_63)  the code is consumed and the block closes;
//   a zero bit from past the data is consumed   the block is finished on zero bits whatever sub_end is, the error
//       is the first of the above that this meets, else ST_DATA_ENDS (ran_dry's rule: at the block's close), and
//       F returns with the block closed, at max(position, sub_end).
// The interval's last subsequence (sub_end == end) never passes through and finishes its block, or decodes one more,
// on zero bits in the same way, so an interval that is short of blocks has the serial decoder's error.  An entry
// state that no decoder can have produced (j, k out of range, a position before sub_begin) is read as (sub_begin, 0,
// 0).  No byte outside [off, end) is read.  With dst (the interval's first coefficient) the non-zero coefficients
// and the DC of blocks first_block + local index < total_blocks are written and decoding stops at total_blocks:
// p0..p2 are the DC predictors on entry.
S2V_JD unsigned long long sync_step(const unsigned char *stream, long off, long end, long sub_begin, long sub_end,
                                    unsigned long long state, const HuffTable *tab, int hs, int vs, int bpm,
                                    SyncSummary &sum, short *dst, long long first_block, long long total_blocks, int p0,
                                    int p1, int p2) {
    sum.blocks = 0;
    sum.dc[0] = sum.dc[1] = sum.dc[2] = 0;
    sum.err = ST_OK;
    sum.err_block = 0;
    long pos = (long)(state >> 16);
    int j = (int)(state >> 8) & 255, k = (int)state & 255;
    if (j >= bpm || k > 63 || pos < sub_begin * 8) {
        pos = sub_begin * 8;
        j = k = 0;
    }
    const long stop = sub_end * 8;
    const bool last = sub_end >= end;
    if (pos >= stop && !last) return sync_pack(pos, j, k);
    PosReader br;
    br.open(stream, off, end, pos);
    unsigned d0 = 0, d1 = 0, d2 = 0;       // the DC differences summed per component: selects, no indexed array
    bool dry = false;
    for (;;) {
        if (dst && (unsigned long long)(first_block + sum.blocks) >= (unsigned long long)total_blocks) break;
        if (!dry && br.position() >= stop) {
            if (!last) break;
            dry = true;
        }
        br.fill();
        const int c = block_component(j, hs, vs);
        short *blk = dst ? dst + (first_block + sum.blocks) * 64 : nullptr;
        int err = ST_OK;
        bool close = false;
        if (k == 0) {
            const int s = huff_decode(br, tab[2 * c]);
            if (s < 0) {
                err = ST_BAD_CODE;
                br.skip(1);
            } else if (s > 11) {
                err = ST_BAD_CODE;
                k = 1;
            } else {
                int diff = 0;
                if (s) {
                    diff = huff_extend((int)br.peek(s), s);
                    br.skip(s);
                }
                unsigned &d = c == 0 ? d0 : (c == 1 ? d1 : d2);
                d += (unsigned)diff;
                if (blk) blk[0] = (short)(int)((unsigned)(c == 0 ? p0 : (c == 1 ? p1 : p2)) + d);
                k = 1;
            }
        } else {
            const int rs = huff_decode(br, tab[2 * c + 1]);
            if (rs < 0) {
                err = ST_BAD_CODE;
                br.skip(1);
            } else {
                const int r = rs >> 4, s = rs & 15;
                if (s == 0) {
                    if (r != 15) {
                        close = true;      // EOB
                    } else if (k + 16 > 63) {
                        err = ST_RUN_PAST_63;
                        close = true;
                    } else {
                        k += 16;
                    }
                } else if (k + r > 63) {
                    err = ST_RUN_PAST_63;
                    close = true;
                } else {
                    k += r;
                    const int v = huff_extend((int)br.peek(s), s);
                    br.skip(s);
                    if (blk) blk[k] = (short)v;
                    close = ++k == 64;
                }
            }
        }
        dry = dry || br.ran_dry();
        if (dry && !err && close) err = ST_DATA_ENDS;
        if (err && !sum.err) {
            sum.err = err;
            sum.err_block = sum.blocks;
        }
        if (close || (dry && err)) {
            ++sum.blocks;
            j = j + 1 == bpm ? 0 : j + 1;
            k = 0;
            if (dry) break;
        }
    }
    sum.dc[0] = (int)d0;
    sum.dc[1] = (int)d1;
    sum.dc[2] = (int)d2;
    const long at = br.position();
    return sync_pack(at > stop ? at : stop, j, k);
}

// subsequences of an interval of ``len`` bytes: at least one, so that an empty interval still raises its status
S2V_JD long sync_subs(long len, int sub_bytes) { return len > 0 ? (len + sub_bytes - 1) / sub_bytes : 1; }
// records the workspace holds behind Dims::total; interval iv's lie at sync_base .. + sync_subs, apart from every
// other interval's when the table is in ascending order and no two intervals overlap
S2V_JD long sync_records(long data_bytes, int n_intervals, int sub_bytes) {
    return data_bytes / sub_bytes + 2L * n_intervals + 2;
}
S2V_JD long sync_base(long off, int iv, int sub_bytes) { return off / sub_bytes + 2L * iv; }

// jidctint's jpeg_idct_islow, one 1-D pass without its rounding shift, in 64-bit integers (libjpeg's JLONG)
S2V_JD void idct_islow_pass(const long long *i, long long *o) {
    long long z1 = (i[2] + i[6]) * 4433;
    const long long t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
    const long long t0 = (i[0] + i[4]) * 8192, t1 = (i[0] - i[4]) * 8192;
    const long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    long long a = i[7], b = i[5], c = i[3], d = i[1];
    z1 = a + d;
    long long z2 = b + c, z3 = a + c, z4 = b + d;
    const long long z5 = (z3 + z4) * 9633;
    a *= 2446;
    b *= 16819;
    c *= 25172;
    d *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a += z1 + z3;
    b += z2 + z4;
    c += z2 + z3;
    d += z1 + z4;
    o[0] = t10 + d;
    o[1] = t11 + c;
    o[2] = t12 + b;
    o[3] = t13 + a;
    o[4] = t13 - a;
    o[5] = t12 - b;
    o[6] = t11 - c;
    o[7] = t10 - d;
}

S2V_JD int clamp_u8(long long v) { return v < 0 ? 0 : (v > 255 ? 255 : (int)v); }

// libjpeg's chroma sample for output pixel (y, x) of a plane c with pitch ``cp`` whose real size is ch x cw:
// hs, vs: luma samples per chroma sample.  h2v2 and h2v1 are the "fancy" triangle filters, edges replicated;
// a plane of cw <= 2 is replicated instead (libjpeg switches to its box filter there); 1x1 is a copy.
S2V_JD int chroma_sample(const unsigned char *c, long cp, int ch, int cw, int hs, int vs, int y, int x) {
    if (hs == 1) return c[(long)y * cp + x];
    const int cx = x >> 1;
    if (cw <= 2) return c[(long)(vs == 2 ? y >> 1 : y) * cp + cx];
    int xn = (x & 1) ? cx + 1 : cx - 1;    // the nearer neighbour column
    xn = xn < 0 ? 0 : (xn > cw - 1 ? cw - 1 : xn);
    if (vs == 1) {
        const unsigned char *r = c + (long)y * cp;
        return (3 * r[cx] + r[xn] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int cy = y >> 1;
    int yn = (y & 1) ? cy + 1 : cy - 1;    // the nearer neighbour row
    yn = yn < 0 ? 0 : (yn > ch - 1 ? ch - 1 : yn);
    const unsigned char *r0 = c + (long)cy * cp, *r1 = c + (long)yn * cp;
    const int s = 3 * r0[cx] + r1[cx], sn = 3 * r0[xn] + r1[xn];
    return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
}

// libjpeg's jdcolor: cb, cr already minus 128
S2V_JD void ycc_to_rgb(int Y, int cb, int cr, int &R, int &G, int &B) {
    R = clamp_u8(Y + ((91881 * cr + 32768) >> 16));
    G = clamp_u8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    B = clamp_u8(Y + ((116130 * cb + 32768) >> 16));
}

// sizes that follow from (h, w, sampling): sampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 (Pillow's numbering)
struct Dims {
    int hs, vs, bpm;               // luma blocks per MCU across and down; blocks per MCU
    int mcols, mrows, mcus;
    int ph, pw, cph, cpw;          // padded luma and chroma plane sizes
    int ch, cw;                    // real chroma size
    long coef_bytes, y_bytes, c_bytes, total;   // per call (n frames); multiples of 16
};

inline bool dims(int n, int h, int w, int sampling, Dims &d) {
    if (n <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535 || sampling < 0 || sampling > 2) return false;
    d.hs = sampling >= 1 ? 2 : 1;
    d.vs = sampling == 2 ? 2 : 1;
    d.bpm = d.hs * d.vs + 2;
    d.mcols = (w + 8 * d.hs - 1) / (8 * d.hs);
    d.mrows = (h + 8 * d.vs - 1) / (8 * d.vs);
    d.mcus = d.mcols * d.mrows;
    d.pw = d.mcols * 8 * d.hs;
    d.ph = d.mrows * 8 * d.vs;
    d.cpw = d.mcols * 8;
    d.cph = d.mrows * 8;
    d.cw = (w + d.hs - 1) / d.hs;
    d.ch = (h + d.vs - 1) / d.vs;
    d.coef_bytes = (long)n * d.mcus * d.bpm * 64 * 2;
    d.y_bytes = (((long)n * d.ph * d.pw) + 15) & ~15L;
    d.c_bytes = (((long)n * d.cph * d.cpw) + 15) & ~15L;
    d.total = d.coef_bytes + d.y_bytes + 2 * d.c_bytes;
    return true;
}

}  // namespace jdec
}  // namespace s2v
