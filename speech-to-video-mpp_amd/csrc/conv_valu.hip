// fp32 VALU convolutions for K <= 64 (conv_smallk, conv_smallk4) and Cout <= 4 (conv_direct_small, conv_small_cpar,
// conv_halo_small), one launch function per family (conv_launch.hpp) that only picks the planner's template instance.
#include "conv_store4.hpp"

#include "conv_launch.hpp"

namespace s2v {

// Small-K direct convolution (K = kh*kw*cin <= 64: the 4-channel image-input layers and the
// 4-channel StyleConv input): tppx threads per pixel group, each QPT x 4 output channels of PX
// consecutive pixels (register blocking over pixels: every weight float4 read from LDS feeds PX
// pixels, 1 LDS byte per FMA at PX = 4 instead of 4); a block walks iters x (256 / tppx) groups of
// one batch entry with that entry's filter [K][cout] staged in LDS once; one float4 of input per
// tap and channel group; fp32 VALU; 16-byte output stores.  These layers are bound by their
// output write; the implicit GEMM pads K to 32 per slice and stages every output tile through LDS
// (3-27 TFLOP/s measured on them).
#ifndef SMALLK_NT
#define SMALLK_NT 1      // streaming (non-temporal) output stores: the image-layer outputs exceed L2 / MALL
#endif
template <int QPT, int PX>
__global__ __launch_bounds__(256) void conv_smallk(ConvArgs a, int batch, int tppx, int iters, int vec) {
    extern __shared__ __attribute__((aligned(16))) float wk[];   // [K][cout]
    const int gpb = 256 / tppx;
    const long long total = (long long)batch * a.M;          // pixels (M % PX == 0: groups stay in one entry)
    const long long g0 = (long long)blockIdx.x * gpb * iters;  // first pixel group of the block
    {
        const long long p0 = g0 * PX;
        const int b0 = (int)((p0 < total ? p0 : 0) / a.M);
        const float *w0 = a.wt + (long long)b0 * a.w_bs;
        // k fastest across lanes: a wave reads whole packed rows (coalesced), LDS gets [K][cout]
        for (int e = threadIdx.x; e < a.K * a.cout; e += 256) {
            const int o = e / a.K, k = e - o * a.K;
            wk[k * a.cout + o] = w0[(long long)o * a.kpad + k];
        }
    }
    __syncthreads();
    const int tq = threadIdx.x % tppx;
    const int hw = a.oh * a.ow;
    for (int it = 0; it < iters; ++it) {
        const long long g = g0 + (long long)it * gpb + threadIdx.x / tppx;
        if (g * PX >= total) break;
        const int bidx = (int)(g * PX / a.M);
        const int mbase = (int)(g * PX - (long long)bidx * a.M);
        const float *x = a.x + (long long)bidx * a.x_bs;
        int img[PX], oy[PX], ox[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            const int m = mbase + p;
            img[p] = m / hw;
            const int rem = m - img[p] * hw;
            oy[p] = rem / a.ow;
            ox[p] = rem - oy[p] * a.ow;
        }
        f4 acc[PX][QPT];
#pragma unroll
        for (int p = 0; p < PX; ++p)
#pragma unroll
            for (int q = 0; q < QPT; ++q) acc[p][q] = f4{0.f, 0.f, 0.f, 0.f};
        for (int ky = 0; ky < a.kh; ++ky)
            for (int kx = 0; kx < a.kw; ++kx) {
                const float *px[PX];
                bool ok[PX];
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    int iy, ix;
                    ok[p] = map_tap(a, oy[p], ox[p], ky, kx, iy, ix);
                    px[p] = x + ((long long)(img[p] * a.h + (ok[p] ? iy : 0)) * a.w + (ok[p] ? ix : 0)) * a.xcs;
                }
                const int kb = (ky * a.kw + kx) * a.cin;
                for (int c = 0; c < a.cin; c += 4) {
                    f4 v[PX];
#pragma unroll
                    for (int p = 0; p < PX; ++p) {
                        v[p] = ok[p] ? *(const f4 *)(px[p] + c) : f4{0.f, 0.f, 0.f, 0.f};
                        if (a.in_scale) v[p] *= *(const f4 *)(a.in_scale + (long long)img[p] * a.in_scale_ns + c);
                        if (a.pre_act) {
                            v[p].x = apply_act(v[p].x, a.pre_act, a.pre_alpha);
                            v[p].y = apply_act(v[p].y, a.pre_act, a.pre_alpha);
                            v[p].z = apply_act(v[p].z, a.pre_act, a.pre_alpha);
                            v[p].w = apply_act(v[p].w, a.pre_act, a.pre_alpha);
                        }
                        if (!ok[p]) v[p] = f4{0.f, 0.f, 0.f, 0.f};   // zero padding stays zero after the prologue
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float *wr = wk + (kb + c + e) * a.cout + 4 * tq;
#pragma unroll
                        for (int q = 0; q < QPT; ++q) {
                            const f4 w4 = *(const f4 *)(wr + 4 * tppx * q);
#pragma unroll
                            for (int p = 0; p < PX; ++p) {
                                const float ve = e == 0 ? v[p].x : e == 1 ? v[p].y : e == 2 ? v[p].z : v[p].w;
                                acc[p][q].x = fmaf(ve, w4.x, acc[p][q].x);
                                acc[p][q].y = fmaf(ve, w4.y, acc[p][q].y);
                                acc[p][q].z = fmaf(ve, w4.z, acc[p][q].z);
                                acc[p][q].w = fmaf(ve, w4.w, acc[p][q].w);
                            }
                        }
                    }
                }
            }
#pragma unroll
        for (int p = 0; p < PX; ++p)
#pragma unroll
            for (int q = 0; q < QPT; ++q)
                store_epilogue4(a, bidx, mbase + p, 4 * (tq + tppx * q), acc[p][q], vec != 0, SMALLK_NT != 0);
    }
}

// 4-channel inputs with a compile-time tap count (1x1 or 3x3: ENet's conv_body_first and the first
// StyleConv on the upsampled 4-channel image): every tap's float4 is loaded before any FMA, so a
// thread has KT loads in flight instead of KT dependent round trips per pixel (the runtime-tap
// loop of conv_smallk ran the 3x3 StyleConv at 0.66 TB/s of output).
template <int QPT, int KT>
__global__ __launch_bounds__(256) void conv_smallk4(ConvArgs a, int batch, int tppx, int iters, int vec) {
    constexpr int KW = KT == 9 ? 3 : 1;
    extern __shared__ __attribute__((aligned(16))) float wk[];   // [K][cout]
    const int gpb = 256 / tppx;
    const long long total = (long long)batch * a.M;
    const long long g0 = (long long)blockIdx.x * gpb * iters;
    {
        const int b0 = (int)((g0 < total ? g0 : 0) / a.M);
        const float *w0 = a.wt + (long long)b0 * a.w_bs;
        for (int e = threadIdx.x; e < KT * 4 * a.cout; e += 256) {   // coalesced packed rows (k fastest)
            const int o = e / (KT * 4), k = e - o * (KT * 4);
            wk[k * a.cout + o] = w0[(long long)o * a.kpad + k];
        }
    }
    __syncthreads();
    const int tq = threadIdx.x % tppx;
    const int hw = a.oh * a.ow;
    if constexpr (KT == 1) {
        // 1x1, one float4 per pixel.  Software-pipelined: pixel u + 1 is loaded before pixel u is
        // stored (vmcnt counts loads and stores in issue order, so a load issued after a store
        // waits for it).  Pixel positions advance incrementally: one division per thread instead
        // of per pixel (the per-pixel 64-bit / 32-bit divisions made this loop VALU-bound, ~190
        // VALU instructions per pixel and wave, 0.65 TB/s of output).
        struct Pos { int b, m, img, oy, ox; };
        auto advance = [&](Pos &p) {
            p.m += gpb;
            p.ox += gpb;
            while (p.ox >= a.ow) { p.ox -= a.ow; ++p.oy; }
            while (p.oy >= a.oh) { p.oy -= a.oh; ++p.img; }
            while (p.img >= a.n) { p.img -= a.n; ++p.b; p.m -= a.M; }
        };
        auto load1 = [&](const Pos &p, f4 &v) {
            const float *x = a.x + (long long)p.b * a.x_bs;
            int iy, ix;
            const bool ok = map_tap(a, p.oy, p.ox, 0, 0, iy, ix);
            v = ok ? *(const f4 *)(x + ((long long)(p.img * a.h + iy) * a.w + ix) * a.xcs) : f4{0.f, 0.f, 0.f, 0.f};
            if (a.in_scale || a.pre_act) {
                v.x = prologue(a, v.x, p.img, 0);
                v.y = prologue(a, v.y, p.img, 1);
                v.z = prologue(a, v.z, p.img, 2);
                v.w = prologue(a, v.w, p.img, 3);
                if (!ok) v = f4{0.f, 0.f, 0.f, 0.f};
            }
        };
        // the epilogue's per-channel scale / shift are loaded once, before any store
        const Epi &ep = a.epi;
        const bool plain = vec && !ep.nc_scale && !ep.res && !ep.pix_add && a.y_step <= 1 && !ep.post_mul && !ep.dup_src;
        f4 esc[QPT], esh[QPT];
#pragma unroll
        for (int q = 0; q < QPT; ++q) {
            const int n = 4 * (tq + tppx * q);
            esc[q] = ep.scale ? *(const f4 *)(ep.scale + n) : f4{1.f, 1.f, 1.f, 1.f};
            esh[q] = ep.shift ? *(const f4 *)(ep.shift + n) : f4{0.f, 0.f, 0.f, 0.f};
        }
        const long long gs = g0 + threadIdx.x / tppx;
        if (gs >= total) return;
        const long long left = (total - gs + gpb - 1) / gpb;
        const int nit = left < iters ? (int)left : iters;
        Pos pl;
        pl.b = (int)(gs / a.M);
        pl.m = (int)(gs - (long long)pl.b * a.M);
        pl.img = pl.m / hw;
        {
            const int rem = pl.m - pl.img * hw;
            pl.oy = rem / a.ow;
            pl.ox = rem - pl.oy * a.ow;
        }
        Pos ps = pl;
        f4 cur = f4{0.f, 0.f, 0.f, 0.f}, nxt = f4{0.f, 0.f, 0.f, 0.f};
        load1(pl, cur);
        for (int it = 0; it < nit; ++it) {
            if (it + 1 < nit) {
                advance(pl);
                load1(pl, nxt);
            }
            f4 acc[QPT];
#pragma unroll
            for (int q = 0; q < QPT; ++q) acc[q] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ve = e == 0 ? cur.x : e == 1 ? cur.y : e == 2 ? cur.z : cur.w;
                const float *wr = wk + e * a.cout + 4 * tq;
#pragma unroll
                for (int q = 0; q < QPT; ++q) {
                    const f4 w4 = *(const f4 *)(wr + 4 * tppx * q);
                    acc[q].x = fmaf(ve, w4.x, acc[q].x);
                    acc[q].y = fmaf(ve, w4.y, acc[q].y);
                    acc[q].z = fmaf(ve, w4.z, acc[q].z);
                    acc[q].w = fmaf(ve, w4.w, acc[q].w);
                }
            }
#pragma unroll
            for (int q = 0; q < QPT; ++q) {
                const int n = 4 * (tq + tppx * q);
                if (!plain) {
                    store_epilogue4(a, ps.b, ps.m, n, acc[q], vec != 0, SMALLK_NT != 0);
                    continue;
                }
                f4 v = acc[q] * esc[q] + esh[q];
                v.x = apply_act(v.x, ep.act, ep.alpha);
                v.y = apply_act(v.y, ep.act, ep.alpha);
                v.z = apply_act(v.z, ep.act, ep.alpha);
                v.w = apply_act(v.w, ep.act, ep.alpha);
                f4 *dst = (f4 *)(a.y + (long long)ps.b * a.y_bs + (long long)ps.m * a.ycs + n);
                if (SMALLK_NT) __builtin_nontemporal_store(v, dst);
                else *dst = v;
            }
            advance(ps);
            cur = nxt;
        }
        return;
    }
    for (int it = 0; it < iters; ++it) {
        const long long g = g0 + (long long)it * gpb + threadIdx.x / tppx;
        if (g >= total) break;
        const int bidx = (int)(g / a.M);
        const int m = (int)(g - (long long)bidx * a.M);
        const float *x = a.x + (long long)bidx * a.x_bs;
        const int img = m / hw, rem = m - img * hw;
        const int oy = rem / a.ow, ox = rem - oy * a.ow;
        f4 v[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            int iy, ix;
            const bool ok = map_tap(a, oy, ox, t / KW, t % KW, iy, ix);
            v[t] = ok ? *(const f4 *)(x + ((long long)(img * a.h + iy) * a.w + ix) * a.xcs) : f4{0.f, 0.f, 0.f, 0.f};
            if (a.in_scale || a.pre_act) {
                v[t].x = prologue(a, v[t].x, img, 0);
                v[t].y = prologue(a, v[t].y, img, 1);
                v[t].z = prologue(a, v[t].z, img, 2);
                v[t].w = prologue(a, v[t].w, img, 3);
                if (!ok) v[t] = f4{0.f, 0.f, 0.f, 0.f};
            }
        }
        f4 acc[QPT];
#pragma unroll
        for (int q = 0; q < QPT; ++q) acc[q] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ve = e == 0 ? v[t].x : e == 1 ? v[t].y : e == 2 ? v[t].z : v[t].w;
                const float *wr = wk + (t * 4 + e) * a.cout + 4 * tq;
#pragma unroll
                for (int q = 0; q < QPT; ++q) {
                    const f4 w4 = *(const f4 *)(wr + 4 * tppx * q);
                    acc[q].x = fmaf(ve, w4.x, acc[q].x);
                    acc[q].y = fmaf(ve, w4.y, acc[q].y);
                    acc[q].z = fmaf(ve, w4.z, acc[q].z);
                    acc[q].w = fmaf(ve, w4.w, acc[q].w);
                }
            }
#pragma unroll
        for (int q = 0; q < QPT; ++q)
            store_epilogue4(a, bidx, m, 4 * (tq + tppx * q), acc[q], vec != 0, SMALLK_NT != 0);
    }
}

void launch_conv_smallk(const ConvArgs &a, int batch, int tppx, int qpt, int kt, int iters, int vec, hipStream_t s) {
    const unsigned grid = cdiv((long long)batch * a.M, (256 / tppx) * iters);
    const size_t lds = (size_t)a.K * a.cout * sizeof(float);
    if (kt == 9 && qpt == 1) conv_smallk4<1, 9><<<grid, 256, lds, s>>>(a, batch, tppx, iters, vec);
    else if (kt == 9) conv_smallk4<2, 9><<<grid, 256, lds, s>>>(a, batch, tppx, iters, vec);
    else if (kt == 1 && qpt == 1) conv_smallk4<1, 1><<<grid, 256, lds, s>>>(a, batch, tppx, iters, vec);
    else if (kt == 1) conv_smallk4<2, 1><<<grid, 256, lds, s>>>(a, batch, tppx, iters, vec);
    else if (qpt == 1) conv_smallk<1, 1><<<grid, 256, lds, s>>>(a, batch, tppx, iters, vec);
    else conv_smallk<2, 1><<<grid, 256, lds, s>>>(a, batch, tppx, iters, vec);
}

// Direct VALU convolution for tiny Cout (final RGB / flow heads, ToRGB): one thread per output
// pixel, all CO outputs per thread.  Per filter tap the block stages W[:, tap, c0:c0+CCH] in LDS,
// so every weight read is an LDS broadcast (all lanes read the same address).
template <int CO>
__global__ __launch_bounds__(256) void conv_direct_small(ConvArgs a, int batch) {
    constexpr int CCH = 512;                  // channels staged per pass
    __shared__ __attribute__((aligned(16))) float wsm[CO * CCH];
    const long long total = (long long)batch * a.M;
    const long long gid = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const bool live = gid < total;
    const int bidx = live ? (int)(gid / a.M) : 0;
    const int m = live ? (int)(gid - (long long)bidx * a.M) : 0;
    const int hw = a.oh * a.ow;
    const int img = m / hw;
    const int rem = m - img * hw;
    const int oy = rem / a.ow, ox = rem - (rem / a.ow) * a.ow;
    const float *x = a.x + (long long)bidx * a.x_bs;
    const float *wt = a.wt + (long long)bidx * a.w_bs;
    float acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = 0.f;
    const bool vec = (a.cin % 4 == 0) && (a.xcs % 4 == 0) && !a.in_scale && !a.pre_act &&
                     (((uintptr_t)x & 15) == 0);
    for (int ky = 0; ky < a.kh; ++ky)
        for (int kx = 0; kx < a.kw; ++kx) {
            int iy = 0, ix = 0;
            const bool ok = live && map_tap(a, oy, ox, ky, kx, iy, ix);
            const float *px = x + ((long long)(img * a.h + iy) * a.w + ix) * a.xcs;
            const int kb = (ky * a.kw + kx) * a.cin;
            for (int c0 = 0; c0 < a.cin; c0 += CCH) {
                const int cn = min(CCH, a.cin - c0);
                __syncthreads();
                for (int e = threadIdx.x; e < CO * cn; e += 256) {
                    const int o = e / cn, c = e - (e / cn) * cn;
                    wsm[o * CCH + c] = o < a.cout ? wt[(long long)o * a.kpad + kb + c0 + c] : 0.f;
                }
                __syncthreads();
                if (!ok) continue;
                if (vec) {
                    for (int c = 0; c < cn; c += 4) {
                        const float4 v = *(const float4 *)(px + c0 + c);
#pragma unroll
                        for (int o = 0; o < CO; ++o) {
                            const float4 wv = *(const float4 *)&wsm[o * CCH + c];
                            acc[o] = fmaf(v.x, wv.x, acc[o]);
                            acc[o] = fmaf(v.y, wv.y, acc[o]);
                            acc[o] = fmaf(v.z, wv.z, acc[o]);
                            acc[o] = fmaf(v.w, wv.w, acc[o]);
                        }
                    }
                } else {
                    for (int c = 0; c < cn; ++c) {
                        const float v = prologue(a, px[c0 + c], img, c0 + c);
#pragma unroll
                        for (int o = 0; o < CO; ++o) acc[o] = fmaf(v, wsm[o * CCH + c], acc[o]);
                    }
                }
            }
        }
    if (!live) return;
#pragma unroll
    for (int o = 0; o < CO; ++o)
        if (o < a.cout) store_epilogue(a, bidx, m, o, acc[o]);
}

// Small-Cout conv, channel-parallel form: TPP lanes share one output pixel, each owns 4 input
// channels (16-byte loads; consecutive lanes read consecutive bytes of the pixel row, so a wave
// reads 64/TPP neighbouring pixels contiguously), partial dot products are combined with
// shuffles.  Requires cin % 4 == 0 and 16-byte aligned rows.
// LW: the block's filter (CO x K floats of one batch entry) is staged in LDS first, so the per-tap
// weight reads are LDS broadcasts instead of CO global loads per input float4.
template <int CO, int TPP, bool LW>
__global__ __launch_bounds__(256) void conv_small_cpar(ConvArgs a, int batch) {
    extern __shared__ __attribute__((aligned(16))) float wsm_dyn[];
    const long long total = (long long)batch * a.M;
    const unsigned blk = xcd_block(blockIdx.x, gridDim.x);      // stencil rows share one XCD's L2
    const long long gid = (blk * 256LL + threadIdx.x) / TPP;
    const int sub = threadIdx.x % TPP;
    const bool live = gid < total;
    const int bidx = live ? (int)(gid / a.M) : 0;
    const int m = live ? (int)(gid - (long long)bidx * a.M) : 0;
    const int hw = a.oh * a.ow;
    const int img = m / hw;
    const int rem = m - img * hw;
    const int oy = rem / a.ow, ox = rem - (rem / a.ow) * a.ow;
    const float *x = a.x + (long long)bidx * a.x_bs;
    const float *wt = a.wt + (long long)bidx * a.w_bs;
    int wstride = a.kpad;
    if (LW) {
        // every pixel of the block belongs to the batch entry of its first pixel (the host
        // guarantees M % (256 / TPP) == 0 when the weights are per batch entry)
        const long long g0 = blk * (256LL / TPP);
        const int b0 = (int)((g0 < total ? g0 : 0) / a.M);
        const float *w0 = a.wt + (long long)b0 * a.w_bs;
        for (int e = threadIdx.x; e < CO * a.K; e += 256) {
            const int o = e / a.K, k = e - (e / a.K) * a.K;
            wsm_dyn[e] = o < a.cout ? w0[(long long)o * a.kpad + k] : 0.f;
        }
        __syncthreads();
        wt = wsm_dyn;
        wstride = a.K;
    }
    float acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = 0.f;
    if (live) {
        for (int ky = 0; ky < a.kh; ++ky)
            for (int kx = 0; kx < a.kw; ++kx) {
                int iy, ix;
                if (!map_tap(a, oy, ox, ky, kx, iy, ix)) continue;
                const float *px = x + ((long long)(img * a.h + iy) * a.w + ix) * a.xcs;
                const int kb = (ky * a.kw + kx) * a.cin;
                for (int c = sub * 4; c < a.cin; c += TPP * 4) {
                    f4 v = *(const f4 *)(px + c);
                    if (a.in_scale) v *= *(const f4 *)(a.in_scale + (long long)img * a.in_scale_ns + c);
                    if (a.pre_act) {
                        v.x = apply_act(v.x, a.pre_act, a.pre_alpha);
                        v.y = apply_act(v.y, a.pre_act, a.pre_alpha);
                        v.z = apply_act(v.z, a.pre_act, a.pre_alpha);
                        v.w = apply_act(v.w, a.pre_act, a.pre_alpha);
                    }
#pragma unroll
                    for (int o = 0; o < CO; ++o) {
                        const f4 wv = *(const f4 *)(wt + (long long)o * wstride + kb + c);
                        acc[o] = fmaf(v.x, wv.x, fmaf(v.y, wv.y, fmaf(v.z, wv.z, fmaf(v.w, wv.w, acc[o]))));
                    }
                }
            }
    }
#pragma unroll
    for (int o = 0; o < CO; ++o)
#pragma unroll
        for (int off = TPP / 2; off > 0; off >>= 1) acc[o] += __shfl_xor(acc[o], off, 64);
    if (!live || sub != 0) return;
#pragma unroll
    for (int o = 0; o < CO; ++o)
        if (o < a.cout) store_epilogue(a, bidx, m, o, acc[o]);
}

template <int CO, int TPP>
static void launch_cpar(const ConvArgs &a, int batch, bool lds_w, hipStream_t s) {
    const unsigned grid = cdiv((long long)batch * a.M * TPP, 256);
    if (lds_w) conv_small_cpar<CO, TPP, true><<<grid, 256, (size_t)CO * a.K * sizeof(float), s>>>(a, batch);
    else conv_small_cpar<CO, TPP, false><<<grid, 256, 0, s>>>(a, batch);
}

template <int CO>
static void launch_small(const ConvArgs &a, int batch, int lanes, bool lds_w, hipStream_t s) {
    switch (lanes) {
        case 0: conv_direct_small<CO><<<cdiv((long long)batch * a.M, 256), 256, 0, s>>>(a, batch); break;
        case 8: launch_cpar<CO, 8>(a, batch, lds_w, s); break;
        case 2: launch_cpar<CO, 2>(a, batch, lds_w, s); break;
        default: launch_cpar<CO, 4>(a, batch, lds_w, s); break;
    }
}

void launch_conv_small(const ConvArgs &a, int batch, int lanes, bool lds_w, hipStream_t s) {
    switch (a.cout) {
        case 1: launch_small<1>(a, batch, lanes, lds_w, s); break;
        case 2: launch_small<2>(a, batch, lanes, lds_w, s); break;
        case 3: launch_small<3>(a, batch, lanes, lds_w, s); break;
        default: launch_small<4>(a, batch, lanes, lds_w, s); break;
    }
}

// Halo-tiled direct conv for Cout <= 4 heads with a wide square filter (DNet's 7x7 64 -> 3 tanh
// head at 256^2, LNet's 7x7 64 -> 3 sigmoid head): a block owns an 8 x 128 output tile; per chunk
// of 4 input channels it stages the (8 + KS - 1) x (128 + KS - 1) input halo once in LDS (planar
// per channel), and each thread computes 4 horizontally adjacent pixels x CO outputs from 16-byte
// LDS row reads, so every staged value feeds up to 4 * KS taps.  The per-pixel gather of
// conv_small_cpar re-read each input pixel KS^2 times from L1/L2 (DNet head: 1.5 ms per 16 frames
// at 185 GB/s).  Filter values are block-uniform (scalar loads).  fp32 VALU, exact products.
template <int CO, int KS>
__global__ __launch_bounds__(256) void conv_halo_small(ConvArgs a, int tiles_x, int tiles_y) {
    constexpr int TH = 8, PX = 4, TW = 32 * PX;
    constexpr int IH = TH + KS - 1, IW = TW + KS - 1, IWP = (IW + 3) / 4 * 4;
    constexpr int NV = (PX + KS - 1 + 3) / 4;                 // float4 row reads per (channel, ky)
    static_assert(4 * 31 + 4 * NV <= IWP, "halo row reads stay inside the padded LDS row");
    __shared__ __attribute__((aligned(16))) float tile[4][IH][IWP];
    const int tid = threadIdx.x, r = tid >> 5, cg = tid & 31;
    int t = blockIdx.x;
    const int txi = t % tiles_x;
    t /= tiles_x;
    const int tyi = t % tiles_y, img = t / tiles_y;
    const int oy0 = tyi * TH, ox0 = txi * TW;
    const float *xb = a.x + (long long)img * a.h * a.w * a.xcs;
    const float *__restrict__ wt = a.wt;
    // channel split (gridDim.y = a.splits, a.tps channels each): raw partial sums to the split-K
    // workspace, folded by splitk_reduce with the epilogue (small images: too few tiles otherwise)
    const int cb = blockIdx.y * a.tps, ce = min(a.cin, cb + a.tps);
    float acc[PX][CO];
#pragma unroll
    for (int p = 0; p < PX; ++p)
#pragma unroll
        for (int o = 0; o < CO; ++o) acc[p][o] = 0.f;
    const bool refl = a.pad_mode == S2V_PAD_REFLECT;
    for (int c0 = cb; c0 < ce; c0 += 4) {
        __syncthreads();                                      // the previous chunk has been consumed
        for (int e = tid; e < IH * IW; e += 256) {
            const int iy = e / IW, ix = e - iy * IW;
            int gy = oy0 + iy - a.ph, gx = ox0 + ix - a.pw;
            if (refl) {
                gy = reflect_idx(gy, a.h);
                gx = reflect_idx(gx, a.w);
            }
            // halo rows / columns past the image (tiles overhanging the bottom / right edge, or
            // beyond a single reflection) feed only outputs that are never stored
            const bool ok = (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
            f4 v = f4{0.f, 0.f, 0.f, 0.f};
            if (ok) v = *(const f4 *)(xb + ((long long)gy * a.w + gx) * a.xcs + c0);
            tile[0][iy][ix] = v.x;
            tile[1][iy][ix] = v.y;
            tile[2][iy][ix] = v.z;
            tile[3][iy][ix] = v.w;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int ky = 0; ky < KS; ++ky) {
                float row[4 * NV];
                const float *src = &tile[c][r + ky][4 * cg];
#pragma unroll
                for (int j = 0; j < NV; ++j) *(f4 *)&row[4 * j] = *(const f4 *)(src + 4 * j);
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) {
                    const long long k = (long long)(ky * KS + kx) * a.cin + c0 + c;
                    float wv[CO];
#pragma unroll
                    for (int o = 0; o < CO; ++o) wv[o] = wt[(long long)o * a.kpad + k];
#pragma unroll
                    for (int p = 0; p < PX; ++p)
#pragma unroll
                        for (int o = 0; o < CO; ++o) acc[p][o] = fmaf(row[p + kx], wv[o], acc[p][o]);
                }
            }
        }
    }
    const int oy = oy0 + r;
    if (oy >= a.oh) return;
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        const int ox = ox0 + 4 * cg + p;
        if (ox >= a.ow) continue;
        const int m = (img * a.oh + oy) * a.ow + ox;
        if (a.splits > 1) {
            float *w = a.ws + ((long long)blockIdx.y * a.M + m) * a.cout;
#pragma unroll
            for (int o = 0; o < CO; ++o) w[o] = acc[p][o];
            continue;
        }
#pragma unroll
        for (int o = 0; o < CO; ++o) store_epilogue(a, 0, m, o, acc[p][o]);
    }
}

template <int CO>
static void launch_halo(const ConvArgs &a, int ks, hipStream_t s) {
    const int tiles_x = (int)cdiv(a.ow, 128), tiles_y = (int)cdiv(a.oh, 8);
    const dim3 grid((unsigned)((long long)a.n * tiles_x * tiles_y), (unsigned)a.splits);
    if (ks == 3) conv_halo_small<CO, 3><<<grid, 256, 0, s>>>(a, tiles_x, tiles_y);
    else if (ks == 5) conv_halo_small<CO, 5><<<grid, 256, 0, s>>>(a, tiles_x, tiles_y);
    else conv_halo_small<CO, 7><<<grid, 256, 0, s>>>(a, tiles_x, tiles_y);
}

void launch_conv_halo_small(const ConvArgs &a, int ks, hipStream_t s) {
    switch (a.cout) {
        case 1: launch_halo<1>(a, ks, s); break;
        case 2: launch_halo<2>(a, ks, s); break;
        case 3: launch_halo<3>(a, ks, s); break;
        default: launch_halo<4>(a, ks, s); break;
    }
}

}  // namespace s2v
