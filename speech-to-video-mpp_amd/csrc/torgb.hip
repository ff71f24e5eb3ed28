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

// x2 bilinear upsample + 3x3 conv from the nine 1x1 tap products of the un-upsampled input (s2v_tapsum_up2):
// the upsample is linear and per channel, so conv3x3(up2(x)) = sum_t shift_t(up2(W_t x)), zero where the shifted
// position leaves the 2h x 2w frame.  P holds W_t x for the nine taps t = 3 dy + dx, tap-major (each tap's Cout
// values of a pixel one contiguous run).
//
// A thread owns one channel quad of one 2 x 2 output cell (frame rows 2k, 2k + 1, columns 2j, 2j + 1).  Away from
// the frame's border the upsampled row q = r + dy - 1 of output row r = 2k + a reads two of the three low-resolution
// rows s0 = k - 1, s1 = k, s2 = k + 1: rows (s0, s1) for a + dy <= 1, else (s1, s2), with weights (0.75, 0.25) when
// a + dy is even and (0.25, 0.75) when odd (up2_index's values there); columns alike.  Tap row dy therefore touches
// 2, 3, 2 low rows: 49 float4 loads feed the cell's 4 x 36 FMAs, with compile-time coefficients, and the cells of a
// wave and of neighbouring waves meet in L1 / L2 for the rest of the reuse.  A cell on the frame's border (clamped
// edge rows of the upsample, taps in the conv's zero padding) takes a rolled per-pixel path with up2_index's own
// taps and weights.  Both sum a pixel in one order: taps 0..8, terms (i0, j0), (i0, j1), (i1, j0), (i1, j1),
// coefficient ly * lx, by fmaf; which path a pixel takes depends on its frame position alone, so a window call
// gives the whole-frame call's bits.
struct TapsumGeo {
    int fh, fw;          // the low-resolution frame
    int ph, pw, sy, sx;  // the P window and its frame position
    int oh, ow, oy, ox;  // the output window and its position in the 2 fh x 2 fw frame
    int k0, j0, ckh, ckw;  // first cell row / column and cell counts of the window
};

struct TapsumEpi {
    const float *noise;
    float pix_w;
    const float *bias;
    float gain;
    int act;
    float alpha;
    float *y;
    int ycs;
};

// interior weight of low row base + ti for an output / tap pair of parity par = (a + d) & 1
__device__ __forceinline__ constexpr float tapsum_w(int par, int ti) { return (par ^ ti) ? 0.25f : 0.75f; }

// Tap (DY, DX) of an interior 2 x 2 cell: the tap's loads (low rows / columns 0..1, 0..2 or 1..2 of the cell's three
// for D = 0, 1, 2), then for each of the four outputs the four bilinear terms in the fixed order
template <int DY, int DX>
__device__ __forceinline__ void tapsum_tap(const float *__restrict__ pt, const long long (&ro)[3], const long long (&co)[3],
                                           float4 (&acc)[2][2]) {
    constexpr int kLo[3] = {0, 0, 1}, kHi[3] = {1, 2, 2};
    float4 v[3][3];
#pragma unroll
    for (int si = 0; si < 3; ++si)
#pragma unroll
        for (int sj = 0; sj < 3; ++sj)
            if (si >= kLo[DY] && si <= kHi[DY] && sj >= kLo[DX] && sj <= kHi[DX])
                v[si][sj] = *(const float4 *)(pt + ro[si] + co[sj]);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            // output row 2k + a reads low rows (base, base + 1): base 0 for a + DY <= 1, else 1; columns alike
            const int bi = a + DY <= 1 ? 0 : 1, bj = c + DX <= 1 ? 0 : 1;
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj) {
                    const float cf = tapsum_w((a + DY) & 1, ti) * tapsum_w((c + DX) & 1, tj);
                    const float4 u = v[bi + ti][bj + tj];
                    acc[a][c].x = fmaf(cf, u.x, acc[a][c].x);
                    acc[a][c].y = fmaf(cf, u.y, acc[a][c].y);
                    acc[a][c].z = fmaf(cf, u.z, acc[a][c].z);
                    acc[a][c].w = fmaf(cf, u.w, acc[a][c].w);
                }
        }
}

// gain, bias, noise, activation and the store of output pixel (wr, wc) of sample b's window
__device__ __forceinline__ void tapsum_store(const TapsumEpi &e, const TapsumGeo &g, int b, int wr, int wc, int quad,
                                             float4 acc) {
    const long long pix = ((long long)b * g.oh + wr) * g.ow + wc;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e.bias) bv = *(const float4 *)(e.bias + quad * 4);
    const float nz = e.noise ? e.pix_w * e.noise[pix] : 0.f;
    float4 r;
    r.x = apply_act(e.gain * acc.x + bv.x + nz, e.act, e.alpha);
    r.y = apply_act(e.gain * acc.y + bv.y + nz, e.act, e.alpha);
    r.z = apply_act(e.gain * acc.z + bv.z + nz, e.act, e.alpha);
    r.w = apply_act(e.gain * acc.w + bv.w + nz, e.act, e.alpha);
    *(float4 *)(e.y + pix * e.ycs + quad * 4) = r;
}

__global__ __launch_bounds__(256) void tapsum_up2_kernel(const float *__restrict__ P, int pcs, int cout, int quads,
                                                         long long items, TapsumEpi e, TapsumGeo g) {
    const long long item = (long long)xcd_block(blockIdx.x, gridDim.x) * 256 + threadIdx.x;
    if (item >= items) return;
    const int quad = (int)(item % quads);
    long long cell = item / quads;
    const int cj = (int)(cell % g.ckw);
    cell /= g.ckw;
    const int ck = (int)(cell % g.ckh);
    const int b = (int)(cell / g.ckh);
    const int k = g.k0 + ck, j = g.j0 + cj;
    const float *pb = P + (long long)b * g.ph * g.pw * pcs + quad * 4;
    if (k >= 1 && k <= g.fh - 2 && j >= 1 && j <= g.fw - 2) {
        // the three low rows / columns at their place in the P window.  The host has checked that every tap of a
        // stored output lies inside the window; a cell half outside the output window clamps its unused taps into it.
        long long ro[3], co[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            ro[s] = (long long)min(max(k + s - 1 - g.sy, 0), g.ph - 1) * g.pw * pcs;
            co[s] = (long long)min(max(j + s - 1 - g.sx, 0), g.pw - 1) * pcs;
        }
        float4 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) acc[a][c] = make_float4(0.f, 0.f, 0.f, 0.f);
        // one tap per trip of a rolled loop: left one basic block, the nine taps' 49 float4 loads are all issued
        // ahead of the first FMA (276 VGPRs, one wave per SIMD); a tap holds at most 9, and a CU's waves overlap
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const float *pt = pb + t * cout;
            switch (t) {
                case 0: tapsum_tap<0, 0>(pt, ro, co, acc); break;
                case 1: tapsum_tap<0, 1>(pt, ro, co, acc); break;
                case 2: tapsum_tap<0, 2>(pt, ro, co, acc); break;
                case 3: tapsum_tap<1, 0>(pt, ro, co, acc); break;
                case 4: tapsum_tap<1, 1>(pt, ro, co, acc); break;
                case 5: tapsum_tap<1, 2>(pt, ro, co, acc); break;
                case 6: tapsum_tap<2, 0>(pt, ro, co, acc); break;
                case 7: tapsum_tap<2, 1>(pt, ro, co, acc); break;
                default: tapsum_tap<2, 2>(pt, ro, co, acc); break;
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int wr = 2 * k + a - g.oy, wc = 2 * j + c - g.ox;   // the pixel's place in the output window
                if ((unsigned)wr < (unsigned)g.oh && (unsigned)wc < (unsigned)g.ow) tapsum_store(e, g, b, wr, wc, quad, acc[a][c]);
            }
        return;
    }
    // a border cell: pixel by pixel, up2_index's taps and weights (the edge clamp), weight zero for a tap row /
    // column in the zero padding; the taps clamped into the P window as above
#pragma unroll 1
    for (int ac = 0; ac < 4; ++ac) {
        const int r = 2 * k + (ac >> 1), c = 2 * j + (ac & 1);
        const int wr = r - g.oy, wc = c - g.ox;
        if ((unsigned)wr >= (unsigned)g.oh || (unsigned)wc >= (unsigned)g.ow) continue;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const int qy = r + t / 3 - 1, qx = c + t % 3 - 1;
            int i0, i1, j0, j1;
            float ly[2], lx[2];
            up2_index(qy, g.fh, i0, i1, ly[0], ly[1]);
            up2_index(qx, g.fw, j0, j1, lx[0], lx[1]);
            if (qy < 0 || qy >= 2 * g.fh) ly[0] = ly[1] = 0.f;
            if (qx < 0 || qx >= 2 * g.fw) lx[0] = lx[1] = 0.f;
            const long long rr[2] = {(long long)min(max(i0 - g.sy, 0), g.ph - 1) * g.pw * pcs,
                                     (long long)min(max(i1 - g.sy, 0), g.ph - 1) * g.pw * pcs};
            const long long cc[2] = {(long long)min(max(j0 - g.sx, 0), g.pw - 1) * pcs,
                                     (long long)min(max(j1 - g.sx, 0), g.pw - 1) * pcs};
            const float *pt = pb + t * cout;
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int tj = 0; tj < 2; ++tj) {
                    const float cf = ly[ti] * lx[tj];
                    const float4 u = *(const float4 *)(pt + rr[ti] + cc[tj]);
                    acc.x = fmaf(cf, u.x, acc.x);
                    acc.y = fmaf(cf, u.y, acc.y);
                    acc.z = fmaf(cf, u.z, acc.z);
                    acc.w = fmaf(cf, u.w, acc.w);
                }
        }
        tapsum_store(e, g, b, wr, wc, quad, acc);
    }
}

}  // namespace s2v

using namespace s2v;

extern "C" int s2v_tapsum_up2(const float *p, int n, int ph, int pw, int pcs, int cout, const float *noise, float pix_w,
                              const float *bias, float gain, int act, float alpha, float *y, int oh, int ow, int ycs,
                              const s2v_tapsum_win *win, s2v_stream_t stream) {
    S2V_REQUIRE(p && y && win && n > 0 && ph > 0 && pw > 0 && oh > 0 && ow > 0 && cout > 0, "tapsum_up2: bad args");
    S2V_REQUIRE(cout % 4 == 0, "tapsum_up2: Cout %d must be a multiple of 4 (16-byte channel accesses)", cout);
    S2V_REQUIRE(act == S2V_ACT_NONE || act == S2V_ACT_LRELU || act == S2V_ACT_RELU, "tapsum_up2: unknown act %d", act);
    const int fh = win->fh > 0 ? win->fh : ph, fw = win->fw > 0 ? win->fw : pw;
    S2V_REQUIRE(fh < (1 << 29) && fw < (1 << 29), "tapsum_up2: frame too large");
    S2V_REQUIRE(win->oy >= 0 && win->ox >= 0 && win->oy + (long long)oh <= 2LL * fh && win->ox + (long long)ow <= 2LL * fw,
                "tapsum_up2: the %dx%d output window at (%d, %d) leaves the %dx%d frame", oh, ow, win->oy, win->ox,
                2 * fh, 2 * fw);
    S2V_REQUIRE(win->sy >= 0 && win->sx >= 0 && win->sy + (long long)ph <= fh && win->sx + (long long)pw <= fw,
                "tapsum_up2: the %dx%d tap-product window at (%d, %d) leaves the %dx%d frame", ph, pw, win->sy, win->sx,
                fh, fw);
    // the low-resolution rows / columns the window's 3x3 taps read: those of upsampled lines o - 1 .. o + len, inside
    // the frame
    int ylo, yhi, xlo, xhi;
    {
        const int qy0 = win->oy > 0 ? win->oy - 1 : 0, qy1 = win->oy + oh < 2 * fh ? win->oy + oh : 2 * fh - 1;
        const int qx0 = win->ox > 0 ? win->ox - 1 : 0, qx1 = win->ox + ow < 2 * fw ? win->ox + ow : 2 * fw - 1;
        up2_tap_range(qy0, qy1 - qy0 + 1, fh, ylo, yhi);
        up2_tap_range(qx0, qx1 - qx0 + 1, fw, xlo, xhi);
    }
    S2V_REQUIRE(ylo >= win->sy && yhi < win->sy + ph && xlo >= win->sx && xhi < win->sx + pw,
                "tapsum_up2: the output window at (%d, %d) reads tap-product rows %d..%d, columns %d..%d: outside the "
                "%dx%d tap-product window at (%d, %d)", win->oy, win->ox, ylo, yhi, xlo, xhi, ph, pw, win->sy, win->sx);
    S2V_REQUIRE(pcs % 4 == 0 && pcs >= 9LL * cout && ycs % 4 == 0 && ycs >= cout,
                "tapsum_up2: pixel pitches must hold 9 Cout / Cout channels and be multiples of 4");
    S2V_REQUIRE(((uintptr_t)p % 16) == 0 && ((uintptr_t)y % 16) == 0 && (!bias || ((uintptr_t)bias % 16) == 0),
                "tapsum_up2: 16-byte aligned p / y / bias");
    S2V_REQUIRE((long long)n * ph * pw * pcs < (1LL << 62) && (long long)n * oh * ow < (1LL << 40),
                "tapsum_up2: problem too large");
    const int k0 = win->oy >> 1, j0 = win->ox >> 1;
    const int ckh = ((win->oy + oh - 1) >> 1) - k0 + 1, ckw = ((win->ox + ow - 1) >> 1) - j0 + 1;
    const int quads = cout / 4;
    const long long items = (long long)n * ckh * ckw * quads;
    const long long blocks = (items + 255) / 256;
    S2V_REQUIRE(blocks < (1LL << 31), "tapsum_up2: grid too large");
    const TapsumGeo g{fh, fw, ph, pw, win->sy, win->sx, oh, ow, win->oy, win->ox, k0, j0, ckh, ckw};
    const TapsumEpi e{noise, noise ? pix_w : 0.f, bias, gain, act, alpha, y, ycs};
    tapsum_up2_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(p, pcs, cout, quads, items, e, g);
    return check_launch("tapsum_up2");
}

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
