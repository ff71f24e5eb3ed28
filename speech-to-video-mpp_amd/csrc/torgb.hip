// ENet / StyleGAN2 ToRGB with its skip upsample in one HBM pass (models/base_blocks.py:536-554:
// ToRGB = ModulatedConv2d(C, 3, 1, demodulate=False) + bias, then + F.interpolate(skip, x2,
// bilinear); ENet.py:119-129 calls it once per decoder stage).
//
//   y[b, p, o] = (sum_c W[o][c] * s[b][c] * x[b, p, c] + bias[o]) + up2(skip)[b, p, o]   o < 3
//   y[b, p, 3] = up2(skip)[b, p, 3]                 (the engine's 4th, float4-padding channel)
//
// The separate path wrote the upsampled skip (16 B / px), then the small-Cout conv read it back as
// its residual and wrote 3 scattered floats per pixel.  Here TPP lanes share a pixel and each owns
// C / TPP channels as float4s (a wave reads 64 / TPP pixel rows, 128-byte pieces), every thread
// carries PPT pixels so ~16 float4 loads are in flight, the modulated 3 x C filter (W * s[b], the
// reference's weight-then-conv order) is built once per block in LDS, partial sums meet by xor
// shuffles, and one lane per pixel reads the 2 x 2 skip taps and writes the pixel as one float4.
// Bound: HBM (C * 4 bytes read + 16 written per output pixel).
//
// s2v_torgb_up2_win runs the pass on a window of a larger frame (ENet's tail computes only what its [8:-8, 8:-8]
// crop keeps): the output pixel's taps and weights are those of its frame position, read at their place in the skip
// window, so a pixel gets bit for bit the whole-frame value; and the finishing lane can store the three channels
// into cropped NCHW planes instead of the float4 pixel (the tail's closing transpose).  A sample is
// ceil(h w / pixels per block) blocks: the last one clamps its loads to the sample's last pixel and skips the
// stores past it, so h * w need not be a multiple of the block.
#include "common.hpp"

namespace s2v {

// torch upsample_bilinear2d (align_corners=False) source index / weights: the resize kernels' rule
__host__ __device__ __forceinline__ void up2_index(int dst, int in, int &i0, int &i1, float &l0, float &l1) {
    float src = 0.5f * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = (int)src;
    i1 = i0 + ((i0 < in - 1) ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}


// Where a launch sits in the full output frame (s2v_torgb_win) and the form of its output
struct TorgbGeo {
    int fsh, fsw;        // the skip frame (half the full output frame): the clamp of the upsample's last tap
    int oy, ox;          // frame position of output pixel (0, 0)
    int sh, sw;          // rows / columns of the skip window
    int sy, sx;          // skip-frame position of skip pixel (0, 0)
    int nchw, cy, cx;    // y as [n][3][H - 2 cy][W - 2 cx] planes instead of 4-channel NHWC pixels
};

template <int TPP, int PPT>
__global__ __launch_bounds__(256) void torgb_up2_kernel(const float *__restrict__ x, int C, int H, int W, int xcs,
                                                        const float *__restrict__ wt, int kpad,
                                                        const float *__restrict__ s, int s_ns,
                                                        const float *__restrict__ bias,
                                                        const float *__restrict__ skip, int skcs,
                                                        float *__restrict__ y, int ycs, int chunks, TorgbGeo g) {
    extern __shared__ __attribute__((aligned(16))) float wm[];      // [3][C]
    constexpr int SLOTS = 256 / TPP, PB = SLOTS * PPT;             // pixels per block
    const int hw = H * W;
    const unsigned blk = xcd_block(blockIdx.x, gridDim.x);
    const int b = (int)(blk / (unsigned)chunks);                    // a block stays in one sample: chunks per sample
    for (int e = threadIdx.x; e < 3 * C; e += 256) {
        const int o = e / C, c = e - o * C;
        wm[e] = wt[(long long)o * kpad + c] * s[(long long)b * s_ns + c];
    }
    __syncthreads();
    const int sub = threadIdx.x % TPP, slot = threadIdx.x / TPP;
    const float *xb = x + (long long)b * hw * xcs;
    const int p0 = (int)(blk - (unsigned)b * (unsigned)chunks) * PB + slot;
    float acc[PPT][3];
#pragma unroll
    for (int i = 0; i < PPT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.f;
    // the pixels past the sample's end (its last block when h * w is no multiple of PB) read the last pixel and
    // write nothing
    int pl[PPT];
#pragma unroll
    for (int i = 0; i < PPT; ++i) pl[i] = min(p0 + i * SLOTS, hw - 1);
    for (int c = sub * 4; c < C; c += 4 * TPP) {
        const float4 w0 = *(const float4 *)&wm[c], w1 = *(const float4 *)&wm[C + c], w2 = *(const float4 *)&wm[2 * C + c];
        float4 v[PPT];
#pragma unroll
        for (int i = 0; i < PPT; ++i) v[i] = *(const float4 *)(xb + (long long)pl[i] * xcs + c);
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            acc[i][0] = fmaf(v[i].x, w0.x, fmaf(v[i].y, w0.y, fmaf(v[i].z, w0.z, fmaf(v[i].w, w0.w, acc[i][0]))));
            acc[i][1] = fmaf(v[i].x, w1.x, fmaf(v[i].y, w1.y, fmaf(v[i].z, w1.z, fmaf(v[i].w, w1.w, acc[i][1]))));
            acc[i][2] = fmaf(v[i].x, w2.x, fmaf(v[i].y, w2.y, fmaf(v[i].z, w2.z, fmaf(v[i].w, w2.w, acc[i][2]))));
        }
    }
#pragma unroll
    for (int i = 0; i < PPT; ++i)
#pragma unroll
        for (int o = 0; o < 3; ++o)
#pragma unroll
            for (int off = TPP / 2; off > 0; off >>= 1) acc[i][o] += __shfl_xor(acc[i][o], off, 64);
    // lane sub == i of the pixel's group finishes pixel i (every lane holds every sum after the butterfly)
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        if (sub != i % TPP) continue;
        const int p = p0 + i * SLOTS;
        if (p >= hw) continue;
        const int oy = p / W, ox = p - (p / W) * W;
        // the taps and weights of the pixel's place in the full frame, read at their place in the skip window
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        up2_index(g.oy + oy, g.fsh, y0, y1, ly0, ly1);
        up2_index(g.ox + ox, g.fsw, x0, x1, lx0, lx1);
        y0 -= g.sy; y1 -= g.sy; x0 -= g.sx; x1 -= g.sx;
        const int sw = g.sw;
        const float *sb = skip + (long long)b * g.sh * sw * skcs;
        const float4 ta = *(const float4 *)(sb + ((long long)y0 * sw + x0) * skcs);
        const float4 tb = *(const float4 *)(sb + ((long long)y0 * sw + x1) * skcs);
        const float4 tc = *(const float4 *)(sb + ((long long)y1 * sw + x0) * skcs);
        const float4 td = *(const float4 *)(sb + ((long long)y1 * sw + x1) * skcs);
        float4 u;
        u.x = ly0 * (lx0 * ta.x + lx1 * tb.x) + ly1 * (lx0 * tc.x + lx1 * td.x);
        u.y = ly0 * (lx0 * ta.y + lx1 * tb.y) + ly1 * (lx0 * tc.y + lx1 * td.y);
        u.z = ly0 * (lx0 * ta.z + lx1 * tb.z) + ly1 * (lx0 * tc.z + lx1 * td.z);
        u.w = ly0 * (lx0 * ta.w + lx1 * tb.w) + ly1 * (lx0 * tc.w + lx1 * td.w);
        float4 r;
        r.x = (acc[i][0] + (bias ? bias[0] : 0.f)) + u.x;
        r.y = (acc[i][1] + (bias ? bias[1] : 0.f)) + u.y;
        r.z = (acc[i][2] + (bias ? bias[2] : 0.f)) + u.z;
        r.w = u.w;
        if (!g.nchw) {
            *(float4 *)(y + ((long long)b * hw + p) * ycs) = r;
        } else {
            const int ph = H - 2 * g.cy, pw = W - 2 * g.cx, qy = oy - g.cy, qx = ox - g.cx;
            if ((unsigned)qy < (unsigned)ph && (unsigned)qx < (unsigned)pw) {
                const long long plane = (long long)ph * pw;
                float *yp = y + (long long)b * 3 * plane + (long long)qy * pw + qx;
                yp[0] = r.x;
                yp[plane] = r.y;
                yp[2 * plane] = r.z;
            }
        }
    }
}

template <int PPT>
static void launch_torgb(unsigned grid, size_t smem, const float *x, int c, int h, int w, int xcs, const float *wt,
                         int kpad, const float *s, int s_ns, const float *bias, const float *skip, int skcs, float *y,
                         int ycs, int chunks, const TorgbGeo &g, hipStream_t st) {
    torgb_up2_kernel<8, PPT><<<grid, 256, smem, st>>>(x, c, h, w, xcs, wt, kpad, s, s_ns, bias, skip, skcs, y, ycs,
                                                      chunks, g);
}

// first and last skip-frame tap of output lines [o, o + len) along one axis (up2_index's rule)
static void up2_tap_range(int o, int len, int in, int &lo, int &hi) {
    int i0, i1;
    float l0, l1;
    up2_index(o, in, i0, i1, l0, l1);
    lo = i0;
    up2_index(o + len - 1, in, i0, i1, l0, l1);
    hi = i1;
}

}  // namespace s2v

using namespace s2v;

extern "C" int s2v_torgb_up2_win(const float *x, int n, int h, int w, int c, int xcs, const float *wt, int kpad,
                                 const float *s, int s_ns, const float *bias, const float *skip, int skcs, float *y,
                                 int ycs, const s2v_torgb_win *win, s2v_stream_t stream) {
    S2V_REQUIRE(x && wt && s && skip && y && win && n > 0 && h > 1 && w > 1 && c > 0, "torgb_up2: bad args");
    const int fh = win->fh > 0 ? win->fh : h, fw = win->fw > 0 ? win->fw : w;
    S2V_REQUIRE(fh % 2 == 0 && fw % 2 == 0, "torgb_up2: output frame %dx%d must be twice the skip frame", fh, fw);
    S2V_REQUIRE(win->oy >= 0 && win->ox >= 0 && win->oy + h <= fh && win->ox + w <= fw,
                "torgb_up2: the %dx%d output window at (%d, %d) leaves the %dx%d frame", h, w, win->oy, win->ox, fh, fw);
    S2V_REQUIRE(win->sh > 0 && win->sw > 0 && win->sy >= 0 && win->sx >= 0 && win->sy + win->sh <= fh / 2 &&
                    win->sx + win->sw <= fw / 2,
                "torgb_up2: the %dx%d skip window at (%d, %d) leaves the %dx%d skip frame", win->sh, win->sw, win->sy,
                win->sx, fh / 2, fw / 2);
    int ylo, yhi, xlo, xhi;
    up2_tap_range(win->oy, h, fh / 2, ylo, yhi);
    up2_tap_range(win->ox, w, fw / 2, xlo, xhi);
    S2V_REQUIRE(ylo >= win->sy && yhi < win->sy + win->sh && xlo >= win->sx && xhi < win->sx + win->sw,
                "torgb_up2: the output window at (%d, %d) reads skip rows %d..%d, columns %d..%d: outside the %dx%d "
                "skip window at (%d, %d)", win->oy, win->ox, ylo, yhi, xlo, xhi, win->sh, win->sw, win->sy, win->sx);
    S2V_REQUIRE(c % 32 == 0 && xcs % 4 == 0 && xcs >= c && kpad >= c && s_ns >= c && skcs % 4 == 0 && skcs >= 4,
                "torgb_up2: C %% 32 == 0, 4-channel skip, float4 pitches required");
    S2V_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)skip % 16) == 0, "torgb_up2: 16-byte aligned x / skip");
    if (win->nchw)
        S2V_REQUIRE(win->cy >= 0 && win->cx >= 0 && 2 * win->cy < h && 2 * win->cx < w,
                    "torgb_up2: crop (%d, %d) leaves nothing of the %dx%d output", win->cy, win->cx, h, w);
    else
        S2V_REQUIRE(ycs % 4 == 0 && ycs >= 4 && ((uintptr_t)y % 16) == 0,
                    "torgb_up2: 4-channel NHWC output, float4 pitch, 16-byte aligned y");
    const long long hw = (long long)h * w;
    S2V_REQUIRE(hw < (1LL << 31) && (long long)n * hw * xcs < (1LL << 62), "torgb_up2: problem too large");
    // ~16 float4 loads in flight per thread: C / 32 per pixel per lane
    int ppt = 16 / (c / 32);
    if (ppt < 1) ppt = 1;
    if (ppt > 4) ppt = 4;
    // whole blocks per sample where a smaller block gives them; otherwise the sample's last block runs part empty
    if (hw % 32 == 0)
        while (ppt > 1 && hw % (32LL * ppt) != 0) ppt >>= 1;
    const long long chunks = (hw + 32LL * ppt - 1) / (32LL * ppt);
    S2V_REQUIRE(chunks * n < (1LL << 31), "torgb_up2: grid too large");
    const unsigned grid = (unsigned)(chunks * n);
    const size_t smem = (size_t)3 * c * sizeof(float);
    const TorgbGeo g{fh / 2, fw / 2, win->oy, win->ox, win->sh, win->sw, win->sy, win->sx, win->nchw ? 1 : 0,
                     win->nchw ? win->cy : 0, win->nchw ? win->cx : 0};
    hipStream_t st = (hipStream_t)stream;
    switch (ppt) {
        case 4: launch_torgb<4>(grid, smem, x, c, h, w, xcs, wt, kpad, s, s_ns, bias, skip, skcs, y, ycs, (int)chunks, g, st); break;
        case 2: launch_torgb<2>(grid, smem, x, c, h, w, xcs, wt, kpad, s, s_ns, bias, skip, skcs, y, ycs, (int)chunks, g, st); break;
        default: launch_torgb<1>(grid, smem, x, c, h, w, xcs, wt, kpad, s, s_ns, bias, skip, skcs, y, ycs, (int)chunks, g, st); break;
    }
    return check_launch("torgb_up2");
}

extern "C" int s2v_torgb_up2(const float *x, int n, int h, int w, int c, int xcs, const float *wt, int kpad,
                             const float *s, int s_ns, const float *bias, const float *skip, int skcs, float *y,
                             int ycs, s2v_stream_t stream) {
    S2V_REQUIRE(h % 2 == 0 && w % 2 == 0, "torgb_up2: output %dx%d must be twice the skip size", h, w);
    const s2v_torgb_win win{h, w, 0, 0, h / 2, w / 2, 0, 0, 0, 0, 0};
    return s2v_torgb_up2_win(x, n, h, w, c, xcs, wt, kpad, s, s_ns, bias, skip, skcs, y, ycs, &win, stream);
}
