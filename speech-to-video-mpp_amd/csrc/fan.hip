// FAN 68-point landmark network pieces around the convs (third_part/face_detection/models.py:13-201,
// utils.py:56-170):
//
//   * the pre-activation passes: every FAN conv reads relu(bn(x)) while the raw x is kept for the
//     residual and the channel concat, so the BN + ReLU of a tensor is its own memory-bound pass
//     (s2v_bn_act_nhwc), fused with the residual sum, the nearest x2 upsample add and the 2x2 average
//     pool that produce the tensor (s2v_fan_merge) so that each tensor is read once for everything
//     derived from it;
//   * utils.crop (the zero-filled window with the reference's 1-based copy bounds, never materialised,
//     then cv2.resize(INTER_LINEAR) on uint8 with the 11-bit fixed-point rule of s2v_resize_linear
//     mode 0) for a batch of faces into the 256x256 network input;
//   * get_preds_fromhm's argmax and quarter-pixel step, read from the NHWC heatmaps as they are.
#include "common.hpp"

namespace s2v {
namespace {

unsigned grid_1d(long long total, int per_block = 256) {
    long long b = (total + per_block - 1) / per_block;
    if (b > 65535LL * 32) b = 65535LL * 32;
    return (unsigned)(b < 1 ? 1 : b);
}

__device__ __forceinline__ float4 ld4(const float *p) { return *(const float4 *)p; }
__device__ __forceinline__ void st4(float *p, float4 v) { *(float4 *)p = v; }
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
// relu(v * s + t), one rounding per channel
__device__ __forceinline__ float4 affine_relu4(float4 v, float4 s, float4 t) {
    return make_float4(fmaxf(fmaf(v.x, s.x, t.x), 0.f), fmaxf(fmaf(v.y, s.y, t.y), 0.f),
                       fmaxf(fmaf(v.z, s.z, t.z), 0.f), fmaxf(fmaf(v.w, s.w, t.w), 0.f));
}

// ------------------------------------------------------------------------------ BN + ReLU
// y[p][c] = relu(x[p][c] * scale[c] + shift[c]) on channel views; one thread per float4 group,
// consecutive threads on consecutive groups of a pixel
__global__ __launch_bounds__(256) void bn_act_nhwc_kernel(const float *__restrict__ x, long long pixels, int c4,
                                                          long long x_cs, const float *__restrict__ scale,
                                                          const float *__restrict__ shift, float *__restrict__ y,
                                                          long long y_cs) {
    const long long total = pixels * c4;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long p = e / c4;
        const int g = (int)(e - p * c4);
        st4(y + p * y_cs + 4 * g, affine_relu4(ld4(x + p * x_cs + 4 * g), ld4(scale + 4 * g), ld4(shift + 4 * g)));
    }
}

// ------------------------------------------------------------------------------ merge
struct FanMerge {
    const float *a, *b;          // b: NULL, [n,h,w,c] or (b_half) [n,h/2,w/2,c] read with nearest x2
    long long a_cs, b_cs;
    int b_half, n, h, w, c4;
    float *s, *sa, *p, *pa;      // outputs (NULL: skipped): s, relu(s*sA+tA), 2x2 mean of s, relu(p*sB+tB)
    long long s_cs, sa_cs, p_cs, pa_cs;
    const float *sA, *tA, *sB, *tB;
};

// QUAD: one thread per (2x2 pixel quad, float4 channel group): the quad's half-size b pixel and its
// pooled outputs belong to that thread alone.  Otherwise one thread per (pixel, group).
template <bool QUAD>
__global__ __launch_bounds__(256) void fan_merge_kernel(FanMerge m) {
    const int qh = QUAD ? m.h / 2 : m.h, qw = QUAD ? m.w / 2 : m.w;
    const long long total = (long long)m.n * qh * qw * m.c4;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int g = (int)(e % m.c4);
        long long t = e / m.c4;
        const int X = (int)(t % qw);
        t /= qw;
        const int Y = (int)(t % qh);
        const long long img = t / qh;
        const int ch = 4 * g;
        float4 sA, tA;
        if (m.sa) {
            sA = ld4(m.sA + ch);
            tA = ld4(m.tA + ch);
        }
        if (!QUAD) {
            const long long px = (img * m.h + Y) * m.w + X;
            float4 v = ld4(m.a + px * m.a_cs + ch);
            if (m.b) v = add4(v, ld4(m.b + px * m.b_cs + ch));
            if (m.s) st4(m.s + px * m.s_cs + ch, v);
            if (m.sa) st4(m.sa + px * m.sa_cs + ch, affine_relu4(v, sA, tA));
            continue;
        }
        const long long qx = (img * qh + Y) * qw + X;
        float4 bh;
        if (m.b && m.b_half) bh = ld4(m.b + qx * m.b_cs + ch);
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long px = (img * m.h + 2 * Y + (k >> 1)) * m.w + 2 * X + (k & 1);
            v[k] = ld4(m.a + px * m.a_cs + ch);
            if (m.b) v[k] = add4(v[k], m.b_half ? bh : ld4(m.b + px * m.b_cs + ch));
            if (m.s) st4(m.s + px * m.s_cs + ch, v[k]);
            if (m.sa) st4(m.sa + px * m.sa_cs + ch, affine_relu4(v[k], sA, tA));
        }
        if (m.p || m.pa) {
            // F.avg_pool2d(s, 2, 2): the four pixels summed pairwise, times the exact 0.25
            const float4 q = add4(add4(v[0], v[1]), add4(v[2], v[3]));
            const float4 mean = make_float4(q.x * 0.25f, q.y * 0.25f, q.z * 0.25f, q.w * 0.25f);
            if (m.p) st4(m.p + qx * m.p_cs + ch, mean);
            if (m.pa) st4(m.pa + qx * m.pa_cs + ch, affine_relu4(mean, ld4(m.sB + ch), ld4(m.tB + ch)));
        }
    }
}

// ------------------------------------------------------------------------------ crop
constexpr int FAN_RES = 256;

// utils.crop (utils.py:107-129) of face f: the (br - ul) window is zero outside the frame and holds
// frame pixel (ul + j) at window index j (what the 1-based newX / oldX copy bounds amount to); it is
// resized to 256x256 by cv2.resize(INTER_LINEAR) on uint8 (resize.cpp: see s2v_resize_linear mode 0).
// table: int32 [faces][5] = (frame, ul.x, ul.y, br.x, br.y).  One thread per output pixel.
__global__ __launch_bounds__(256) void fan_crop_kernel(const unsigned char *__restrict__ frames, int H, int W,
                                                       const int *__restrict__ table, int faces,
                                                       float *__restrict__ y) {
    const long long total = (long long)faces * FAN_RES * FAN_RES;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int X = (int)(e % FAN_RES), Y = (int)((e / FAN_RES) % FAN_RES), f = (int)(e / (FAN_RES * FAN_RES));
        const int *t = table + 5 * f;
        const int ulx = t[1], uly = t[2];
        const int ww = t[3] - ulx, wh = t[4] - uly;
        const unsigned char *img = frames + (long long)t[0] * H * W * 3;
        const double sx = 1.0 / ((double)FAN_RES / ww), sy = 1.0 / ((double)FAN_RES / wh);
        float fx = (float)((X + 0.5) * sx - 0.5);
        int x0 = (int)floorf(fx);
        fx -= (float)x0;
        if (x0 < 0) { x0 = 0; fx = 0.f; }
        if (x0 >= ww - 1) { x0 = ww - 1; fx = 0.f; }
        const int x1 = min(x0 + 1, ww - 1);
        float fy = (float)((Y + 0.5) * sy - 0.5);
        const int yy = (int)floorf(fy);
        fy -= (float)yy;
        const int y0 = min(max(yy, 0), wh - 1), y1 = min(max(yy + 1, 0), wh - 1);
        const int a0 = __float2int_rn((1.f - fx) * 2048.f), a1 = __float2int_rn(fx * 2048.f);
        const int b0 = __float2int_rn((1.f - fy) * 2048.f), b1 = __float2int_rn(fy * 2048.f);
        // window index -> frame index, or -1 where the window is zero
        const int fx0 = ulx + x0, fx1 = ulx + x1, fy0 = uly + y0, fy1 = uly + y1;
        const bool okx0 = fx0 >= 0 && fx0 < W, okx1 = fx1 >= 0 && fx1 < W;
        const bool oky0 = fy0 >= 0 && fy0 < H, oky1 = fy1 >= 0 && fy1 < H;
        float4 out;
        float *o = &out.x;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int p00 = (oky0 && okx0) ? img[((long long)fy0 * W + fx0) * 3 + ch] : 0;
            const int p01 = (oky0 && okx1) ? img[((long long)fy0 * W + fx1) * 3 + ch] : 0;
            const int p10 = (oky1 && okx0) ? img[((long long)fy1 * W + fx0) * 3 + ch] : 0;
            const int p11 = (oky1 && okx1) ? img[((long long)fy1 * W + fx1) * 3 + ch] : 0;
            const int d0 = p00 * a0 + p01 * a1, d1 = p10 * a0 + p11 * a1;
            const int v = min(max(((((d0 >> 4) * b0) >> 16) + (((d1 >> 4) * b1) >> 16) + 2) >> 2, 0), 255);
            o[ch] = (float)v / 255.f;
        }
        out.w = 0.f;
        st4(y + e * 4, out);
    }
}

// ------------------------------------------------------------------------------ peaks
constexpr int HM = 64;               // get_preds_fromhm's border test is written for 64x64 maps
constexpr int PEAK_WAVES = 16;

// One block per (image, 64-channel chunk): lane = channel, so a wave reads one pixel's channel row
// coalesced; wave v scans pixels v, v + 16, ... in ascending order keeping the first maximum, the 16
// partial results are reduced through LDS (greater value, then lower index: torch.max's first
// maximum), and wave 0 applies the +-0.25 step and the -0.5.
__global__ __launch_bounds__(64 * PEAK_WAVES) void fan_peaks_kernel(const float *__restrict__ hm, int c, long long cs,
                                                                   float *__restrict__ preds,
                                                                   float *__restrict__ vals) {
    __shared__ float sv[PEAK_WAVES][64];
    __shared__ int si[PEAK_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ch = blockIdx.y * 64 + lane;
    const float *map = hm + (long long)blockIdx.x * HM * HM * cs;
    float best = -INFINITY;
    int idx = HM * HM;
    if (ch < c) {
#pragma unroll 8
        for (int p = wave; p < HM * HM; p += PEAK_WAVES) {
            const float v = map[(long long)p * cs + ch];
            if (v > best || idx == HM * HM) {
                best = v;
                idx = p;
            }
        }
    }
    sv[wave][lane] = best;
    si[wave][lane] = idx;
    __syncthreads();
    if (wave != 0 || ch >= c) return;
    for (int k = 1; k < PEAK_WAVES; ++k) {
        const float v = sv[k][lane];
        const int i = si[k][lane];
        if (v > best || (v == best && i < idx)) {
            best = v;
            idx = i;
        }
    }
    const int pX = idx % HM, pY = idx / HM;
    float px = (float)(pX + 1), py = (float)(pY + 1);
    if (pX > 0 && pX < 63 && pY > 0 && pY < 63) {
        const float dx = map[((long long)pY * HM + pX + 1) * cs + ch] - map[((long long)pY * HM + pX - 1) * cs + ch];
        const float dy = map[((long long)(pY + 1) * HM + pX) * cs + ch] - map[((long long)(pY - 1) * HM + pX) * cs + ch];
        px += dx > 0.f ? 0.25f : dx < 0.f ? -0.25f : 0.f;
        py += dy > 0.f ? 0.25f : dy < 0.f ? -0.25f : 0.f;
    }
    const long long o = (long long)blockIdx.x * c + ch;
    preds[2 * o] = px - 0.5f;
    preds[2 * o + 1] = py - 0.5f;
    vals[o] = best;
}

bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace s2v

using namespace s2v;

extern "C" int s2v_bn_act_nhwc(const float *x, long long pixels, int c, long long x_cs, int x_off, const float *scale,
                               const float *shift, float *y, long long y_cs, int y_off, s2v_stream_t stream) {
    S2V_REQUIRE(x && y && scale && shift && pixels > 0 && c > 0, "bn_act_nhwc: bad args");
    S2V_REQUIRE(c % 4 == 0, "bn_act_nhwc: %d channels (a multiple of 4)", c);
    S2V_REQUIRE(x_off >= 0 && y_off >= 0 && x_off % 4 == 0 && y_off % 4 == 0 && x_cs % 4 == 0 && y_cs % 4 == 0 &&
                    x_off + (long long)c <= x_cs && y_off + (long long)c <= y_cs,
                "bn_act_nhwc: channel views [%d, +%d) of pitch %lld and [%d, +%d) of pitch %lld must be multiples of 4 "
                "inside their pitches", x_off, c, x_cs, y_off, c, y_cs);
    S2V_REQUIRE(al16(x) && al16(y) && al16(scale) && al16(shift), "bn_act_nhwc: pointers must be 16-byte aligned");
    S2V_REQUIRE(pixels * (c / 4) < (1LL << 40), "bn_act_nhwc: problem too large");
    bn_act_nhwc_kernel<<<grid_1d(pixels * (c / 4)), 256, 0, (hipStream_t)stream>>>(x + x_off, pixels, c / 4, x_cs, scale,
                                                                                   shift, y + y_off, y_cs);
    return check_launch("bn_act_nhwc");
}

extern "C" int s2v_fan_merge(const float *a, long long a_cs, const float *b, long long b_cs, int b_half, int n, int h,
                             int w, int c, float *s, long long s_cs, float *sa, long long sa_cs, const float *scale_a,
                             const float *shift_a, float *p, long long p_cs, float *pa, long long pa_cs,
                             const float *scale_b, const float *shift_b, s2v_stream_t stream) {
    S2V_REQUIRE(a && n > 0 && h > 0 && w > 0 && c > 0 && (b_half == 0 || b_half == 1), "fan_merge: bad args");
    S2V_REQUIRE(s || sa || p || pa, "fan_merge: no output");
    S2V_REQUIRE(b || !b_half, "fan_merge: b_half without b");
    S2V_REQUIRE(c % 4 == 0 && a_cs % 4 == 0 && a_cs >= c, "fan_merge: %d channels / pitch %lld (multiples of 4, pitch >= "
                "channels)", c, a_cs);
    S2V_REQUIRE(!b || (b_cs % 4 == 0 && b_cs >= c), "fan_merge: b pitch %lld", b_cs);
    S2V_REQUIRE(!s || (s_cs % 4 == 0 && s_cs >= c), "fan_merge: s pitch %lld", s_cs);
    S2V_REQUIRE(!sa || (sa_cs % 4 == 0 && sa_cs >= c && scale_a && shift_a), "fan_merge: activated output needs its "
                "pitch (%lld) and scale / shift", sa_cs);
    S2V_REQUIRE(!p || (p_cs % 4 == 0 && p_cs >= c), "fan_merge: p pitch %lld", p_cs);
    S2V_REQUIRE(!pa || (pa_cs % 4 == 0 && pa_cs >= c && scale_b && shift_b), "fan_merge: activated pooled output needs "
                "its pitch (%lld) and scale / shift", pa_cs);
    const bool quad = b_half || p || pa;
    S2V_REQUIRE(!quad || (h % 2 == 0 && w % 2 == 0), "fan_merge: the pooled outputs and a half-size b need even sizes, "
                "got %dx%d", h, w);
    S2V_REQUIRE(al16(a) && al16(b) && al16(s) && al16(sa) && al16(p) && al16(pa) && al16(scale_a) && al16(shift_a) &&
                    al16(scale_b) && al16(shift_b), "fan_merge: pointers must be 16-byte aligned");
    S2V_REQUIRE((long long)n * h * w * (c / 4) < (1LL << 40), "fan_merge: problem too large");
    FanMerge m;
    m.a = a; m.b = b; m.a_cs = a_cs; m.b_cs = b_cs; m.b_half = b_half;
    m.n = n; m.h = h; m.w = w; m.c4 = c / 4;
    m.s = s; m.sa = sa; m.p = p; m.pa = pa;
    m.s_cs = s_cs; m.sa_cs = sa_cs; m.p_cs = p_cs; m.pa_cs = pa_cs;
    m.sA = scale_a; m.tA = shift_a; m.sB = scale_b; m.tB = shift_b;
    hipStream_t st = (hipStream_t)stream;
    if (quad) fan_merge_kernel<true><<<grid_1d((long long)n * (h / 2) * (w / 2) * m.c4), 256, 0, st>>>(m);
    else fan_merge_kernel<false><<<grid_1d((long long)n * h * w * m.c4), 256, 0, st>>>(m);
    return check_launch("fan_merge");
}

extern "C" int s2v_fan_crop(const unsigned char *frames, int n, int h, int w, const int *table, const int *host_table,
                            int faces, float *y, s2v_stream_t stream) {
    S2V_REQUIRE(frames && table && host_table && y && n > 0 && h > 0 && w > 0 && faces > 0, "fan_crop: bad args");
    S2V_REQUIRE(al16(y), "fan_crop: y must be 16-byte aligned");
    S2V_REQUIRE((long long)h * w * 3 * n < (1LL << 40), "fan_crop: frames too large");
    for (int f = 0; f < faces; ++f) {
        const int *t = host_table + 5 * f;
        S2V_REQUIRE(t[0] >= 0 && t[0] < n, "fan_crop: face %d names frame %d of %d", f, t[0], n);
        bool ok = t[3] > t[1] && t[4] > t[2];
        for (int k = 1; k < 5; ++k) ok = ok && t[k] > -(1 << 24) && t[k] < (1 << 24);
        S2V_REQUIRE(ok, "fan_crop: face %d has an empty or oversized window (ul %d,%d br %d,%d)", f, t[1], t[2], t[3],
                    t[4]);
    }
    fan_crop_kernel<<<grid_1d((long long)faces * FAN_RES * FAN_RES), 256, 0, (hipStream_t)stream>>>(frames, h, w, table,
                                                                                                     faces, y);
    return check_launch("fan_crop");
}

extern "C" int s2v_fan_peaks(const float *hm, int n, int h, int w, int c, long long cs, float *preds, float *vals,
                             s2v_stream_t stream) {
    S2V_REQUIRE(hm && preds && vals && n > 0 && c > 0, "fan_peaks: bad args");
    S2V_REQUIRE(h == HM && w == HM, "fan_peaks: %dx%d maps (get_preds_fromhm's border rule is for 64x64)", h, w);
    S2V_REQUIRE(cs >= c && c <= 65535 * 64, "fan_peaks: pitch %lld < %d channels", cs, c);
    fan_peaks_kernel<<<dim3((unsigned)n, (unsigned)((c + 63) / 64)), 64 * PEAK_WAVES, 0, (hipStream_t)stream>>>(
        hm, c, cs, preds, vals);
    return check_launch("fan_peaks");
}
