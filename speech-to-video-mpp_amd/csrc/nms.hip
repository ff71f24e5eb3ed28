// Batched exact greedy NMS over the compacted candidate buffers of s2v_s3fd_decode (8 floats per row)
// and s2v_retina_decode (16 floats per row), where they lie: utils/nms/py_cpu_nms.py:10-37 and
// detection/sfd/bbox.py:44-64 with a defined order among equal scores.
//
//   1. rows with !(score > min_score) are dropped;
//   2. the rest are ordered by score descending, the larger position index first among equal scores
//      (np.argsort(kind="stable")[::-1] on position-ordered rows);
//   3. top_k > 0: only the first top_k rows take part;
//   4. the greedy sweep, fp32, unfused, in the reference's expression order;
//   5. the kept rows are copied whole, in keep order.
//
// One 256-thread workgroup per image.  The 64-bit keys (orderable score bits << 32 | position index)
// and the 24-bit slot of each row are bitonic-sorted in LDS; the boxes of the sorted rows are then
// gathered into the key array's place.  An image with more rows than the sort holds, of which only the first
// top_k <= capacity take part, is cut to those rows first: an 8-bit radix select of the top_k-th key over the
// rows in global memory (8 histogram passes).  The sweep goes in chunks of 64 sorted rows: wave 0 resolves a
// chunk against itself with ballot masks, then every wave applies the chunk's kept rows to all later
// rows (two barriers per chunk).  Nothing depends on the slot a row arrived in.
#include "common.hpp"

#pragma clang fp contract(off)

namespace s2v {
namespace {

constexpr int NMS_CAPACITY = 8192;   // rows per image that fit the LDS sort (19 B per row: box + 24-bit slot)
constexpr int NMS_THREADS = 256;

// LDS carve (bytes) for npad rows (a power of two, >= 64): every offset a multiple of 16
struct NmsCarve {
    size_t slots, slots_hi, supp, prefix, misc, total;
};

inline NmsCarve nms_carve(int npad) {
    NmsCarve c;
    c.slots = (size_t)npad * 16;                 // [0, slots): keys (8 B) during the sort, boxes (16 B) after it
    c.slots_hi = c.slots + (size_t)npad * 2;     // [slots, slots_hi): bits 0-15 of each row's slot
    c.supp = c.slots_hi + (size_t)npad;          // [slots_hi, supp): bits 16-23 of it
    c.prefix = c.supp + (size_t)(npad / 64) * 8; // [supp, prefix): one bit per sorted row: suppressed
    c.misc = c.prefix + (((size_t)(npad / 64) * 4 + 15) & ~(size_t)15);   // [prefix, misc): kept rows before a chunk
    c.total = c.misc + 32;                       // [misc, total): counters
    return c;
}

// !(ovr <= thresh): row b does not survive kept row a (a NaN ovr suppresses, as np.where(ovr <= thresh))
__device__ __forceinline__ bool nms_suppresses(const float4 a, const float area_a, const float4 b, const float area_b,
                                               const float thresh) {
    const float xx1 = fmaxf(a.x, b.x), yy1 = fmaxf(a.y, b.y);
    const float xx2 = fminf(a.z, b.z), yy2 = fminf(a.w, b.w);
    const float w = fmaxf(0.f, xx2 - xx1 + 1.f), h = fmaxf(0.f, yy2 - yy1 + 1.f);
    const float inter = w * h;
    const float ovr = inter / (area_a + area_b - inter);
    return !(ovr <= thresh);
}

__device__ __forceinline__ float nms_area(const float4 b) { return (b.z - b.x + 1.f) * (b.w - b.y + 1.f); }

// the sort key of row r (orderable score bits << 32 | position index); false when step 1 drops the row
__device__ __forceinline__ bool nms_key(const float *rows, int r, int rs, float min_score, unsigned long long &key) {
    const float s = rows[(long long)r * rs + 5];
    if (!(s > min_score)) return false;
    unsigned u = s == 0.f ? 0u : __float_as_uint(s);                     // -0 orders as +0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    key = ((unsigned long long)u << 32) | (unsigned)__float_as_int(rows[(long long)r * rs]);
    return true;
}

__global__ __launch_bounds__(NMS_THREADS) void nms_kernel(const float *__restrict__ cand, const int *__restrict__ count,
                                                          int max_cand, int rs, float iou_thresh, float min_score,
                                                          int top_k, int keep_max, int npad_max, NmsCarve carve,
                                                          float *__restrict__ out, int *__restrict__ kept,
                                                          int *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long *keys = (unsigned long long *)smem;
    float4 *boxes = (float4 *)smem;
    unsigned short *slots = (unsigned short *)(smem + carve.slots);
    unsigned char *slots_hi = (unsigned char *)(smem + carve.slots_hi);
    unsigned long long *supp = (unsigned long long *)(smem + carve.supp);
    int *prefix = (int *)(smem + carve.prefix);
    int *misc = (int *)(smem + carve.misc);          // [0] rows after the filter, [1] a NaN score was seen,
                                                     // [2] the select's rows still to find, [4..5] its key prefix
    unsigned long long *sel = (unsigned long long *)(misc + 4);
    int *hist = (int *)smem;                         // the select's 256 bins, before any key is stored

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *rows = cand + (long long)b * max_cand * rs;
    int cnt = count[b];
    cnt = cnt < 0 ? 0 : (cnt > max_cand ? max_cand : cnt);
    const int cap = npad_max < NMS_CAPACITY ? npad_max : NMS_CAPACITY;   // rows this launch's LDS can order

    if (tid < 2) misc[tid] = 0;
    __syncthreads();

    // ---- 1. filter + keys
    for (int r = tid; r < cnt; r += NMS_THREADS) {
        const float s = rows[(long long)r * rs + 5];
        if (s != s) misc[1] = 1;
        unsigned long long key;
        if (!nms_key(rows, r, rs, min_score, key)) continue;
        const int at = atomicAdd(&misc[0], 1);
        if (at >= cap) continue;
        keys[at] = key;
        slots[at] = (unsigned short)r;
        slots_hi[at] = (unsigned char)(r >> 16);
    }
    __syncthreads();
    int m = misc[0];
    const bool nan_seen = misc[1] != 0;
    if (!nan_seen && m > cap && top_k > 0 && top_k <= cap) {
        // ---- 3 before 2: more rows than the sort holds, but only the first top_k take part.  Find the
        // top_k-th largest key a byte at a time, from the top: count the rows whose higher bytes equal the
        // prefix found so far by their next byte, and walk the bins down to the one holding the row sought.
        if (tid == 0) {
            misc[2] = top_k;
            *sel = 0ull;
        }
        for (int byte = 7; byte >= 0; --byte) {
            hist[tid] = 0;                                               // 256 threads, 256 bins
            __syncthreads();
            const unsigned long long pre = *sel;
            for (int r = tid; r < cnt; r += NMS_THREADS) {
                unsigned long long key;
                if (!nms_key(rows, r, rs, min_score, key)) continue;
                if (byte < 7 && (key >> (8 * (byte + 1))) != pre) continue;
                atomicAdd(&hist[(int)((key >> (8 * byte)) & 255ull)], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int left = misc[2], d = 255;
                while (d > 0 && hist[d] < left) left -= hist[d--];
                misc[2] = left;
                *sel = (pre << 8) | (unsigned long long)d;
            }
            __syncthreads();
        }
        const unsigned long long kth = *sel;
        if (tid == 0) misc[0] = 0;
        __syncthreads();
        for (int r = tid; r < cnt; r += NMS_THREADS) {
            unsigned long long key;
            if (!nms_key(rows, r, rs, min_score, key) || key < kth) continue;
            const int at = atomicAdd(&misc[0], 1);
            if (at >= cap) continue;                                     // only rows of one key can overflow here
            keys[at] = key;
            slots[at] = (unsigned short)r;
            slots_hi[at] = (unsigned char)(r >> 16);
        }
        __syncthreads();
        m = misc[0];
    }
    if (nan_seen || m > cap) {
        if (tid == 0) {
            status[b] = nan_seen ? 2 : 1;
            kept[b] = 0;
        }
        return;
    }
    if (m == 0) {
        if (tid == 0) {
            status[b] = 0;
            kept[b] = 0;
        }
        return;
    }
    int npad = 64;
    while (npad < m) npad <<= 1;
    for (int i = m + tid; i < npad; i += NMS_THREADS) {
        keys[i] = 0ull;                                                  // below every real key
        slots[i] = 0;
        slots_hi[i] = 0;
    }
    __syncthreads();

    // ---- 2. bitonic sort, descending
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (npad >> 1); t += NMS_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));     // the lower index of pair t
                const int p = i | j;
                const unsigned long long a = keys[i], c = keys[p];
                const bool desc = (i & k) == 0;
                if (desc ? a < c : a > c) {
                    keys[i] = c;
                    keys[p] = a;
                    const unsigned short sa = slots[i];
                    slots[i] = slots[p];
                    slots[p] = sa;
                    const unsigned char ha = slots_hi[i];
                    slots_hi[i] = slots_hi[p];
                    slots_hi[p] = ha;
                }
            }
            __syncthreads();
        }
    }

    // ---- 3. top_k, and the boxes of the sorted rows over the keys (dead since the sort's last barrier)
    const int M = (top_k > 0 && top_k < m) ? top_k : m;
    const int nchunk = (M + 63) >> 6;
    for (int r = tid; r < M; r += NMS_THREADS) {
        const float *row = rows + (long long)((int)slots[r] | ((int)slots_hi[r] << 16)) * rs;
        boxes[r] = make_float4(row[1], row[2], row[3], row[4]);
    }
    for (int i = tid; i < nchunk; i += NMS_THREADS) supp[i] = 0ull;
    __syncthreads();

    // ---- 4. the sweep
    for (int c = 0; c < nchunk; ++c) {
        const int c0 = c << 6;
        if (wave == 0) {
            const int r = c0 + lane;
            const bool valid = r < M;
            const float4 me = boxes[valid ? r : c0];
            const float area_me = nms_area(me);
            const int nj = M - c0 < 64 ? M - c0 : 64;
            unsigned long long dead = supp[c];                           // suppressed by earlier chunks
            if (nj < 64) dead |= ~0ull << nj;
            const unsigned long long alive = ~dead;                      // only these rows can be kept and suppress
            unsigned long long by = 0ull;                                // bit j: row c0 + j (j < lane) suppresses me
            for (unsigned long long kk = alive; kk; kk &= kk - 1) {
                const int j = __ffsll((long long)kk) - 1;
                const float4 o = boxes[c0 + j];
                const bool s = j < lane && nms_suppresses(o, nms_area(o), me, area_me, iou_thresh);
                by |= s ? 1ull << j : 0ull;
            }
            for (unsigned long long kk = alive; kk; kk &= kk - 1) {
                const int j = __ffsll((long long)kk) - 1;
                const unsigned long long col = __ballot((by >> j) & 1ull);
                if (!((dead >> j) & 1ull)) dead |= col;                  // row j is kept: it removes its column
            }
            if (lane == 0) supp[c] = dead;
        }
        __syncthreads();
        const unsigned long long keep = ~supp[c];
        if (keep != 0ull && c + 1 < nchunk) {
            for (int base = c0 + 64; base < M; base += NMS_THREADS) {
                const int r = base + tid;
                const int word = r >> 6;
                bool s = false;
                if (r < M && !((supp[word] >> (r & 63)) & 1ull)) {
                    const float4 me = boxes[r];
                    const float area_me = nms_area(me);
                    unsigned long long kk = keep;
                    while (kk && !s) {
                        const int j = __ffsll((long long)kk) - 1;
                        kk &= kk - 1;
                        const float4 o = boxes[c0 + j];
                        s = nms_suppresses(o, nms_area(o), me, area_me, iou_thresh);
                    }
                }
                const unsigned long long hit = __ballot(s);              // base is a multiple of 64: one word per wave
                if (lane == 0 && hit && base + (wave << 6) < M) supp[word] |= hit;
            }
        }
        __syncthreads();
    }

    // ---- 5. output: kept rows whole, in keep order
    if (tid == 0) {
        int acc = 0;
        for (int i = 0; i < nchunk; ++i) {
            prefix[i] = acc;
            acc += __popcll(~supp[i]);
        }
        kept[b] = acc;
        status[b] = 0;
    }
    __syncthreads();
    const unsigned *src = (const unsigned *)rows;
    unsigned *dst = (unsigned *)(out + (long long)b * keep_max * rs);
    for (int e = tid; e < M * rs; e += NMS_THREADS) {
        const int r = e / rs, f = e - r * rs;
        const unsigned long long w = supp[r >> 6];
        if ((w >> (r & 63)) & 1ull) continue;
        const int rank = prefix[r >> 6] + __popcll(~w & ((1ull << (r & 63)) - 1ull));
        if (rank >= keep_max) continue;
        dst[(long long)rank * rs + f] = src[(long long)((int)slots[r] | ((int)slots_hi[r] << 16)) * rs + f];
    }
}

}  // namespace
}  // namespace s2v

using namespace s2v;

extern "C" int s2v_nms_capacity(void) { return NMS_CAPACITY; }

extern "C" int s2v_nms(const float *cand, const int *count, int n, int max_cand, int row_stride, float iou_thresh,
                       float min_score, int top_k, int keep_max, float *out, int *kept, int *status,
                       s2v_stream_t stream) {
    S2V_REQUIRE(cand && count && out && kept && status, "nms: null pointer");
    S2V_REQUIRE(n > 0 && max_cand > 0 && keep_max > 0 && top_k >= 0, "nms: n %d, max_cand %d, keep_max %d, top_k %d", n,
                max_cand, keep_max, top_k);
    S2V_REQUIRE(row_stride >= 6 && row_stride <= 64, "nms: row_stride %d (6 to 64 floats per row)", row_stride);
    S2V_REQUIRE(iou_thresh == iou_thresh && min_score == min_score, "nms: NaN threshold");
    // the sorted rows remember their slot in 24 bits
    S2V_REQUIRE(max_cand <= (1 << 24), "nms: max_cand %d (at most 2^24 rows per image)", max_cand);
    S2V_REQUIRE((long long)max_cand * row_stride < (1LL << 31) && (long long)keep_max * row_stride < (1LL << 31),
                "nms: rows too long");
    int npad = 64;
    while (npad < max_cand && npad < NMS_CAPACITY) npad <<= 1;           // no image can order more than this
    const NmsCarve carve = nms_carve(npad);
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void *)nms_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr = true;
    }
    nms_kernel<<<n, NMS_THREADS, carve.total, (hipStream_t)stream>>>(cand, count, max_cand, row_stride, iou_thresh,
                                                                     min_score, top_k, keep_max, npad, carve, out, kept,
                                                                     status);
    return check_launch("nms");
}
