// Baseline JPEG decoder (ITU T.81, 8-bit YCbCr 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan) over a batch of
// streams: the contract of include/s2v.h (s2v_jpeg_decode), all in integers, equal to libjpeg's default decoder
// (JDCT_ISLOW, fancy upsampling).  The arithmetic lives in jpeg_dec_core.hpp, which tools/jpeg_decode_host.cpp
// compiles for the host.
//
//   1. jpeg_entropy_decode: the unit of work is one restart interval (the host's table of them spans the batch).
//      Huffman decoding inside an interval is serial, so one lane decodes; the two kernels differ in what the
//      other 63 do.  _wave: one wave per interval; the wave derives the frame's six code tables (maxcode /
//      valptr / huffval and an 8-bit look-ahead) into LDS, and per block zeroes 64 LDS coefficients, lets lane 0
//      decode into them and stores them as one 128-byte row.  _lane: one lane per interval, 64 intervals of one
//      frame per wave, straight into the zeroed workspace.  A bad code, a run past 63 or data that ends early
//      ends the interval and raises the frame's status.  _sync (s2v_jpeg_decode_sync) decodes inside an interval
//      in parallel, for streams without restart markers: see the kernel.
//   2. jpeg_idct: one wave per MCU.  Lane (u, v) dequantises coefficient (u, v) of every block into LDS; lane
//      (block, column) runs the column pass, lane (block, row) the row pass and the clamp; the planes are stored
//      four samples at a time at their MCU-padded sizes.
//   3. jpeg_upsample_color: one thread per output pixel: the fancy chroma filter over the real chroma size (it
//      reads neighbour MCUs, hence its own launch) and YCbCr -> RGB, three bytes into the caller's frame.
#include "common.hpp"
#include "jpeg_dec_core.hpp"

namespace s2v {
namespace {

using namespace jdec;

constexpr int JD_WAVE = 64;
constexpr int JI_THREADS = 256;            // idct: 4 waves, one MCU each
constexpr int JS_THREADS = 1024;           // sync: 16 waves, four per SIMD, to hide each other's dependent loads

// natural index u * 8 + v of zigzag position z
__constant__ unsigned char c_nat_of_zz[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the six code tables of set ``set`` into LDS, by the whole workgroup (>= 6 threads)
__device__ __forceinline__ void derive_tables(const EntropyArgs &a, int set, HuffTable *tab) {
    const unsigned char *spec = a.huff_sets + (long)set * HUFF_SET_BYTES;
    const int tid = threadIdx.x;
    if (tid < HUFF_SET_TABLES) huff_derive_codes(spec + tid * HUFF_SPEC_BYTES, tab[tid]);
    __syncthreads();
    for (int i = tid; i < HUFF_SET_TABLES * 256; i += blockDim.x)
        huff_derive_entry(spec + (i >> 8) * HUFF_SPEC_BYTES, tab[i >> 8], i & 255);
    __syncthreads();
}

__global__ __launch_bounds__(JD_WAVE) void jpeg_entropy_decode_wave(EntropyArgs a) {
    __shared__ HuffTable s_tab[HUFF_SET_TABLES];
    __shared__ short s_blk[64];
    __shared__ int s_err;
    const int lane = threadIdx.x;
    const Interval iv = load_interval(a, blockIdx.x);
    if (!iv.ok) {                          // a table the host did not build: every frame is suspect
        for (int b = lane; b < a.n; b += JD_WAVE) atomicMax(&a.status[b], (int)ST_BAD_TABLE);
        return;
    }
    const int set = a.set_index[iv.frame];
    if (set < 0 || set >= a.n_sets) {
        if (lane == 0) atomicMax(&a.status[iv.frame], (int)ST_BAD_TABLE);
        return;
    }
    derive_tables(a, set, s_tab);
    BitReader br;
    br.open(a.stream, iv.off, iv.end);
    int p0 = 0, p1 = 0, p2 = 0;
    short *dst = a.coef + ((long)iv.frame * a.mcus + iv.first) * a.bpm * 64;
    const int blocks = iv.count * a.bpm;
    int j = 0;
    for (int k = 0; k < blocks; ++k) {
        s_blk[lane] = 0;
        __syncthreads();
        if (lane == 0) {
            const int c = block_component(j, a.hs, a.vs);
            int &pred = c == 0 ? p0 : (c == 1 ? p1 : p2);
            s_err = decode_block(br, s_tab[2 * c], s_tab[2 * c + 1], pred, s_blk);
        }
        __syncthreads();
        dst[(long)k * 64 + lane] = s_blk[lane];
        const int err = s_err;
        if (err != ST_OK) {                // uniform: the interval ends here
            if (lane == 0) atomicMax(&a.status[iv.frame], err);
            return;
        }
        j = j + 1 == a.bpm ? 0 : j + 1;
    }
}

// grid (ceil(max intervals per frame / 64), n); the workspace's coefficients are zero on entry
__global__ __launch_bounds__(JD_WAVE) void jpeg_entropy_decode_lane(EntropyArgs a) {
    __shared__ HuffTable s_tab[HUFF_SET_TABLES];
    const int lane = threadIdx.x, frame = blockIdx.y;
    const int lo = a.frame_first[frame], hi = a.frame_first[frame + 1];
    const int set = a.set_index[frame];
    if (lo < 0 || hi < lo || hi > a.n_intervals || set < 0 || set >= a.n_sets) {
        if (lane == 0 && blockIdx.x == 0) atomicMax(&a.status[frame], (int)ST_BAD_TABLE);
        return;
    }
    if ((long)blockIdx.x * JD_WAVE >= hi - lo) return;
    derive_tables(a, set, s_tab);
    const int idx = lo + blockIdx.x * JD_WAVE + lane;
    if (idx >= hi) return;
    const Interval iv = load_interval(a, idx);
    if (!iv.ok || iv.frame != frame) {
        atomicMax(&a.status[frame], (int)ST_BAD_TABLE);
        return;
    }
    const int err = decode_interval(a, iv, s_tab);
    if (err != ST_OK) atomicMax(&a.status[frame], err);
}

// The sync split (jpeg_dec_core.hpp, sync_step): one workgroup per interval, one lane per subsequence, a lane
// taking every JS_THREADS-th subsequence when the interval has more.  rec: sync_records() records behind the
// planes, as four arrays: the states t of this round and of the next, the entry state each lane last decoded from,
// and its summary.  Resolve: t[0] is true, t[b] starts as (first bit of b, 0, 0); a round sets next[b + 1] =
// F_b(t[b]) for every b (a lane whose entry state did not change keeps its exit state without decoding) and the
// rounds end when one changes nothing: after round r, t[0..r + 1] are the serial decoder's states, so nsub + 1 rounds
// always suffice and the loop is bounded by them.  Write: an exclusive scan of the summaries gives each lane its
// first block and DC predictors, and a last F from the true states stores the coefficients into the zeroed
// workspace.  The interval's status is the error at the lowest block index below count * bpm.  The barriers are the
// workgroup's own: no workgroup waits for another.  Each workgroup checks its interval against its predecessor only:
// when some pair of the table is out of order every frame gets status 4, and the other workgroups still run, perhaps
// on records that overlap another interval's.  What they then read is racing garbage, and that is safe by
// construction, not by luck: sync_step reads any 64 bits as a state (out-of-range fields become the subsequence's
// start), the rounds are bounded by nsub + 1 whatever the states do, and every coefficient store is behind an
// unsigned block index < count * bpm test, so nothing leaves the frame's coefficients.
__global__ __launch_bounds__(JS_THREADS) void jpeg_entropy_decode_sync(EntropyArgs a, int sub, unsigned long long *rec,
                                                                       long n_rec) {
    __shared__ HuffTable s_tab[HUFF_SET_TABLES];
    __shared__ long long s_blk[JS_THREADS];
    __shared__ int s_dc[3][JS_THREADS];
    __shared__ unsigned long long s_first_err;
    const int tid = threadIdx.x;
    const Interval iv = load_interval(a, blockIdx.x);
    bool ok = iv.ok;
    if (ok && blockIdx.x > 0) {            // ascending and apart: what keeps the intervals' records apart
        const Interval before = load_interval(a, blockIdx.x - 1);
        ok = before.ok && iv.off >= before.end;
    }
    const long nsub = ok ? sync_subs(iv.end - iv.off, sub) : 0;
    const long base = ok ? sync_base(iv.off, blockIdx.x, sub) : 0;
    if (!ok || base + nsub + 1 > n_rec) {
        for (int b = tid; b < a.n; b += JS_THREADS) atomicMax(&a.status[b], (int)ST_BAD_TABLE);
        return;
    }
    const int set = a.set_index[iv.frame];
    if (set < 0 || set >= a.n_sets) {
        if (tid == 0) atomicMax(&a.status[iv.frame], (int)ST_BAD_TABLE);
        return;
    }
    derive_tables(a, set, s_tab);
    unsigned long long *cur = rec + base, *nxt = rec + n_rec + base, *seen = rec + 2 * n_rec + base;
    SyncSummary *sums = (SyncSummary *)(rec + 3 * n_rec) + base;
    for (long b = tid; b <= nsub; b += JS_THREADS) {
        cur[b] = nxt[b] = sync_pack((iv.off + b * sub) * 8, 0, 0);
        if (b < nsub) seen[b] = ~0ULL;     // no state: a position has 48 bits
    }
    if (tid == 0) s_first_err = ~0ULL;
    __syncthreads();
    SyncSummary sum;
    for (long round = 0; round <= nsub; ++round) {
        int changed = 0;
        for (long b = tid; b < nsub; b += JS_THREADS) {
            const unsigned long long in = cur[b];
            unsigned long long out = cur[b + 1];
            if (in != seen[b]) {
                const long lo = iv.off + b * sub, hi = lo + sub < iv.end ? lo + sub : iv.end;
                out = sync_step(a.stream, iv.off, iv.end, lo, hi, in, s_tab, a.hs, a.vs, a.bpm, sum, nullptr, 0, 0, 0, 0,
                                0);
                seen[b] = in;
                sums[b] = sum;
            }
            nxt[b + 1] = out;
            changed |= out != cur[b + 1];
        }
        unsigned long long *t = cur;
        cur = nxt;
        nxt = t;
        if (!__syncthreads_or(changed)) break;
    }
    short *dst = a.coef + ((long)iv.frame * a.mcus + iv.first) * a.bpm * 64;
    const long long total = (long long)iv.count * a.bpm;
    long long first = 0;                   // of this pass's first subsequence; uniform
    int p0 = 0, p1 = 0, p2 = 0;
    for (long b0 = 0; b0 < nsub; b0 += JS_THREADS) {
        const long b = b0 + tid;
        const bool live = b < nsub;
        if (live) sum = sums[b];
        s_blk[tid] = live ? sum.blocks : 0;
        for (int c = 0; c < 3; ++c) s_dc[c][tid] = live ? sum.dc[c] : 0;
        __syncthreads();
        for (int d = 1; d < JS_THREADS; d <<= 1) {             // inclusive scan
            long long vb = 0;
            int v0 = 0, v1 = 0, v2 = 0;
            if (tid >= d) {
                vb = s_blk[tid - d];
                v0 = s_dc[0][tid - d];
                v1 = s_dc[1][tid - d];
                v2 = s_dc[2][tid - d];
            }
            __syncthreads();
            s_blk[tid] += vb;
            s_dc[0][tid] = (int)((unsigned)s_dc[0][tid] + (unsigned)v0);
            s_dc[1][tid] = (int)((unsigned)s_dc[1][tid] + (unsigned)v1);
            s_dc[2][tid] = (int)((unsigned)s_dc[2][tid] + (unsigned)v2);
            __syncthreads();
        }
        if (live) {
            const long long mine = first + s_blk[tid] - sum.blocks;
            const int q0 = (int)((unsigned)p0 + (unsigned)s_dc[0][tid] - (unsigned)sum.dc[0]);
            const int q1 = (int)((unsigned)p1 + (unsigned)s_dc[1][tid] - (unsigned)sum.dc[1]);
            const int q2 = (int)((unsigned)p2 + (unsigned)s_dc[2][tid] - (unsigned)sum.dc[2]);
            const unsigned long long at = (unsigned long long)(mine + sum.err_block);
            if (sum.err != ST_OK && at < (unsigned long long)total) atomicMin(&s_first_err, at << 3 | (unsigned)sum.err);
            if ((unsigned long long)mine < (unsigned long long)total) {
                const long lo = iv.off + b * sub, hi = lo + sub < iv.end ? lo + sub : iv.end;
                SyncSummary unused;
                sync_step(a.stream, iv.off, iv.end, lo, hi, cur[b], s_tab, a.hs, a.vs, a.bpm, unused, dst, mine, total,
                          q0, q1, q2);
            }
        }
        first += s_blk[JS_THREADS - 1];
        p0 = (int)((unsigned)p0 + (unsigned)s_dc[0][JS_THREADS - 1]);
        p1 = (int)((unsigned)p1 + (unsigned)s_dc[1][JS_THREADS - 1]);
        p2 = (int)((unsigned)p2 + (unsigned)s_dc[2][JS_THREADS - 1]);
        __syncthreads();
    }
    if (tid == 0 && s_first_err != ~0ULL) atomicMax(&a.status[iv.frame], (int)(s_first_err & 7));
}

__global__ __launch_bounds__(JI_THREADS) void jpeg_idct(const short *__restrict__ coef,
                                                        const unsigned short *__restrict__ qt, int mcols, int mcus,
                                                        int hs, int vs, int bpm, int ph, int pw, int cph, int cpw,
                                                        unsigned char *__restrict__ yp, unsigned char *__restrict__ cbp,
                                                        unsigned char *__restrict__ crp) {
    __shared__ int s_a[4][6][64];
    __shared__ int s_b[4][6][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    const int mcu_raw = blockIdx.x * 4 + wave;
    const bool live = mcu_raw < mcus;
    const int mcu = live ? mcu_raw : mcus - 1;
    const int my = mcu / mcols, mx = mcu - my * mcols;
    const short *src = coef + ((long)b * mcus + mcu) * bpm * 64;
    const int nat = c_nat_of_zz[lane];      // lane = zigzag position: a coalesced row of coefficients
    for (int blk = 0; blk < bpm; ++blk) {
        const int comp = block_component(blk, hs, vs);
        s_a[wave][blk][nat] = (int)src[blk * 64 + lane] * (int)qt[((long)b * 3 + comp) * 64 + lane];
    }
    __syncthreads();
    const int blk = lane >> 3, t = lane & 7;
    if (blk < bpm) {                        // columns: (x + 1024) >> 11
        long long in[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = s_a[wave][blk][r * 8 + t];
        idct_islow_pass(in, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) s_b[wave][blk][r * 8 + t] = (int)((o[r] + 1024) >> 11);
    }
    __syncthreads();
    if (blk < bpm) {                        // rows: (x + 2^17) >> 18, + 128, clamp
        long long in[8], o[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) in[c] = s_b[wave][blk][t * 8 + c];
        idct_islow_pass(in, o);
#pragma unroll
        for (int c = 0; c < 8; ++c) s_a[wave][blk][t * 8 + c] = clamp_u8(((o[c] + (1LL << 17)) >> 18) + 128);
    }
    __syncthreads();
    if (!live) return;
    for (int it = lane; it < bpm * 16; it += 64) {          // four samples of one block row per lane
        const int k = it >> 4, r = (it >> 1) & 7, half = it & 1;
        const int *p = s_a[wave][k] + r * 8 + half * 4;
        const unsigned v = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
        const int comp = block_component(k, hs, vs);
        unsigned char *dst;
        if (comp == 0) {
            const int by = k / hs, bx = k - by * hs;
            dst = yp + ((long)b * ph + my * 8 * vs + by * 8 + r) * pw + mx * 8 * hs + bx * 8 + half * 4;
        } else {
            dst = (comp == 1 ? cbp : crp) + ((long)b * cph + my * 8 + r) * cpw + mx * 8 + half * 4;
        }
        *(unsigned *)dst = v;               // planes are 16-byte aligned, pitches multiples of 8
    }
}

__global__ __launch_bounds__(256) void jpeg_upsample_color(const unsigned char *__restrict__ yp,
                                                           const unsigned char *__restrict__ cbp,
                                                           const unsigned char *__restrict__ crp, int h, int w, int hs,
                                                           int vs, int ph, int pw, int cph, int cpw, int ch, int cw,
                                                           unsigned char *__restrict__ out, long pitch,
                                                           long frame_stride, int bgr) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    if (x >= w || y >= h) return;
    const int Y = yp[((long)b * ph + y) * pw + x];
    const long coff = (long)b * cph * cpw;
    const int cb = chroma_sample(cbp + coff, cpw, ch, cw, hs, vs, y, x) - 128;
    const int cr = chroma_sample(crp + coff, cpw, ch, cw, hs, vs, y, x) - 128;
    int R, G, B;
    ycc_to_rgb(Y, cb, cr, R, G, B);
    unsigned char *q = out + (long)b * frame_stride + (long)y * pitch + (long)x * 3;
    q[0] = (unsigned char)(bgr ? B : R);
    q[1] = (unsigned char)G;
    q[2] = (unsigned char)(bgr ? R : B);
}

}  // namespace
}  // namespace s2v

using namespace s2v;

extern "C" long s2v_jpeg_decode_ws_bytes(int n, int h, int w, int sampling) {
    jdec::Dims d;
    return jdec::dims(n, h, w, sampling, d) ? d.total : 0;
}

static long sync_rec_bytes(long data_bytes, int n_intervals, int sub_bytes) {
    return (jdec::sync_records(data_bytes, n_intervals, sub_bytes) * jdec::SYNC_RECORD_BYTES + 15) & ~15L;
}

extern "C" long s2v_jpeg_decode_sync_ws_bytes(int n, int h, int w, int sampling, long data_bytes, int n_intervals,
                                              int sub_bytes) {
    jdec::Dims d;
    if (!jdec::dims(n, h, w, sampling, d) || data_bytes <= 0 || n_intervals <= 0 || sub_bytes < jdec::SYNC_SUB_MIN ||
        sub_bytes > jdec::SYNC_SUB_MAX || sub_bytes % 4)
        return 0;
    return d.total + sync_rec_bytes(data_bytes, n_intervals, sub_bytes);
}

extern "C" int s2v_jpeg_decode_sync(const uint8_t *data, long data_bytes, const int *intervals, int n_intervals,
                                    const int *frame_first, int max_per_frame, int n, int h, int w, int sampling,
                                    const uint16_t *qtables, const uint8_t *huff_sets, int n_sets, const int *set_index,
                                    uint8_t *out, long pitch_bytes, long frame_stride_bytes, int bgr, int *status,
                                    void *ws, long ws_bytes, int sub_bytes, s2v_stream_t stream) {
    S2V_REQUIRE(data && intervals && frame_first && qtables && huff_sets && set_index && out && status && ws,
                "jpeg_decode_sync: null pointer");
    jdec::Dims d;
    S2V_REQUIRE(n <= 65535 && jdec::dims(n, h, w, sampling, d), "jpeg_decode_sync: n %d, h %d, w %d, sampling %d", n, h,
                w, sampling);
    S2V_REQUIRE(data_bytes > 0 && n_intervals > 0 && max_per_frame > 0 && max_per_frame <= n_intervals && n_sets > 0,
                "jpeg_decode_sync: data_bytes %ld, n_intervals %d, max_per_frame %d, n_sets %d", data_bytes,
                n_intervals, max_per_frame, n_sets);
    S2V_REQUIRE(pitch_bytes >= 3L * w && frame_stride_bytes >= 0,
                "jpeg_decode_sync: pitch %ld (>= 3 w), frame stride %ld", pitch_bytes, frame_stride_bytes);
    S2V_REQUIRE(bgr == 0 || bgr == 1, "jpeg_decode_sync: bgr %d (0 or 1)", bgr);
    S2V_REQUIRE(sub_bytes >= jdec::SYNC_SUB_MIN && sub_bytes <= jdec::SYNC_SUB_MAX && sub_bytes % 4 == 0,
                "jpeg_decode_sync: sub_bytes %d (a multiple of 4 from %d to %d)", sub_bytes, jdec::SYNC_SUB_MIN,
                jdec::SYNC_SUB_MAX);
    const long need = d.total + sync_rec_bytes(data_bytes, n_intervals, sub_bytes);
    S2V_REQUIRE(ws_bytes >= need && ((size_t)ws & 15) == 0,
                "jpeg_decode_sync: workspace %ld bytes (need %ld, 16-byte aligned)", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    short *coef = (short *)ws;
    unsigned char *yp = (unsigned char *)ws + d.coef_bytes, *cbp = yp + d.y_bytes, *crp = cbp + d.c_bytes;
    unsigned long long *rec = (unsigned long long *)((unsigned char *)ws + d.total);
    if (hipMemsetAsync(status, 0, sizeof(int) * (size_t)n, st) != hipSuccess) return check_launch("jpeg_decode_sync");
    if (hipMemsetAsync(coef, 0, (size_t)d.coef_bytes, st) != hipSuccess) return check_launch("jpeg_decode_sync");
    EntropyArgs a{data, data_bytes, intervals, n_intervals, frame_first, n, d.mcus, d.hs, d.vs, d.bpm,
                  huff_sets, n_sets, set_index, coef, status};
    jpeg_entropy_decode_sync<<<dim3(n_intervals), JS_THREADS, 0, st>>>(
        a, sub_bytes, rec, jdec::sync_records(data_bytes, n_intervals, sub_bytes));
    jpeg_idct<<<dim3(cdiv(d.mcus, 4), n), JI_THREADS, 0, st>>>(coef, qtables, d.mcols, d.mcus, d.hs, d.vs, d.bpm, d.ph,
                                                              d.pw, d.cph, d.cpw, yp, cbp, crp);
    jpeg_upsample_color<<<dim3(cdiv(w, 64), cdiv(h, 4), n), dim3(64, 4), 0, st>>>(
        yp, cbp, crp, h, w, d.hs, d.vs, d.ph, d.pw, d.cph, d.cpw, d.ch, d.cw, out, pitch_bytes, frame_stride_bytes, bgr);
    return check_launch("jpeg_decode_sync");
}

extern "C" int s2v_jpeg_decode(const uint8_t *data, long data_bytes, const int *intervals, int n_intervals,
                               const int *frame_first, int max_per_frame, int n, int h, int w, int sampling,
                               const uint16_t *qtables, const uint8_t *huff_sets, int n_sets, const int *set_index,
                               uint8_t *out, long pitch_bytes, long frame_stride_bytes, int bgr, int *status, void *ws,
                               long ws_bytes, int split, s2v_stream_t stream) {
    S2V_REQUIRE(data && intervals && frame_first && qtables && huff_sets && set_index && out && status && ws,
                "jpeg_decode: null pointer");
    jdec::Dims d;
    S2V_REQUIRE(n <= 65535 && jdec::dims(n, h, w, sampling, d), "jpeg_decode: n %d, h %d, w %d, sampling %d", n, h, w,
                sampling);
    S2V_REQUIRE(data_bytes > 0 && n_intervals > 0 && max_per_frame > 0 && max_per_frame <= n_intervals && n_sets > 0,
                "jpeg_decode: data_bytes %ld, n_intervals %d, max_per_frame %d, n_sets %d", data_bytes, n_intervals,
                max_per_frame, n_sets);
    S2V_REQUIRE(pitch_bytes >= 3L * w && frame_stride_bytes >= 0, "jpeg_decode: pitch %ld (>= 3 w), frame stride %ld",
                pitch_bytes, frame_stride_bytes);
    S2V_REQUIRE(bgr == 0 || bgr == 1, "jpeg_decode: bgr %d (0 or 1)", bgr);
    S2V_REQUIRE(split == 0 || split == 1, "jpeg_decode: split %d (0: a wave per interval, 1: a lane)", split);
    S2V_REQUIRE(ws_bytes >= d.total && ((size_t)ws & 15) == 0, "jpeg_decode: workspace %ld bytes (need %ld, 16-byte aligned)",
                ws_bytes, d.total);
    hipStream_t st = (hipStream_t)stream;
    short *coef = (short *)ws;
    unsigned char *yp = (unsigned char *)ws + d.coef_bytes, *cbp = yp + d.y_bytes, *crp = cbp + d.c_bytes;
    if (hipMemsetAsync(status, 0, sizeof(int) * (size_t)n, st) != hipSuccess) return check_launch("jpeg_decode");
    EntropyArgs a{data, data_bytes, intervals, n_intervals, frame_first, n, d.mcus, d.hs, d.vs, d.bpm,
                  huff_sets, n_sets, set_index, coef, status};
    if (split == 0) {
        jpeg_entropy_decode_wave<<<dim3(n_intervals), JD_WAVE, 0, st>>>(a);
    } else {
        if (hipMemsetAsync(coef, 0, (size_t)d.coef_bytes, st) != hipSuccess) return check_launch("jpeg_decode");
        jpeg_entropy_decode_lane<<<dim3(cdiv(max_per_frame, JD_WAVE), n), JD_WAVE, 0, st>>>(a);
    }
    jpeg_idct<<<dim3(cdiv(d.mcus, 4), n), JI_THREADS, 0, st>>>(coef, qtables, d.mcols, d.mcus, d.hs, d.vs, d.bpm, d.ph,
                                                              d.pw, d.cph, d.cpw, yp, cbp, crp);
    jpeg_upsample_color<<<dim3(cdiv(w, 64), cdiv(h, 4), n), dim3(64, 4), 0, st>>>(
        yp, cbp, crp, h, w, d.hs, d.vs, d.ph, d.pw, d.cph, d.cpw, d.ch, d.cw, out, pitch_bytes, frame_stride_bytes, bgr);
    return check_launch("jpeg_decode");
}
