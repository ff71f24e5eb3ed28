// The 16-byte epilogue store shared by the split-K folds (conv.hip) and the small-K VALU kernels (conv_valu.hip).
#pragma once
#include "conv_impl.hpp"

namespace s2v {

// Epilogue of 4 consecutive output channels [n, n + 4) of row m as one 16-byte store (host
// guarantees 16-byte aligned rows: ycs, res_cs % 4 == 0; n % 4 == 0); per-element otherwise.
__device__ __forceinline__ void store_epilogue4(const ConvArgs &a, int bidx, int m, int n, f4 v, bool vec,
                                                bool nt) {
    const Epi &e = a.epi;
    if (!vec || e.nc_scale || (e.res && !e.res_simple) || a.y_step > 1) {
        store_epilogue(a, bidx, m, n + 0, v.x);
        store_epilogue(a, bidx, m, n + 1, v.y);
        store_epilogue(a, bidx, m, n + 2, v.z);
        store_epilogue(a, bidx, m, n + 3, v.w);
        return;
    }
    if (e.scale) v *= *(const f4 *)(e.scale + n);
    if (e.shift) v += *(const f4 *)(e.shift + n);
    if (e.pix_add) v += e.pix_w * e.pix_add[pix_index(a, bidx, m, n)];
    f4 r = {0.f, 0.f, 0.f, 0.f};
    if (e.res) {
        r = *(const f4 *)(e.res + (long long)bidx * a.res_bs + (long long)m * e.res_cs + n);
        if (!e.res_after) v += r;
    }
    v.x = apply_act(v.x, e.act, e.alpha);
    v.y = apply_act(v.y, e.act, e.alpha);
    v.z = apply_act(v.z, e.act, e.alpha);
    v.w = apply_act(v.w, e.act, e.alpha);
    if (e.res && e.res_after) v += r;
    if (e.post_mul && n >= e.post_c0) {       // SFT (post_c0 % 4 == 0 under vec: a quad is all in or out)
        const long long q = (long long)m * e.post_cs + n - e.post_c0;
        v = v * *(const f4 *)(e.post_mul + q) + *(const f4 *)(e.post_add + q);
    }
    f4 *dst = (f4 *)(a.y + (long long)bidx * a.y_bs + (long long)m * a.ycs + n);
    if (nt) __builtin_nontemporal_store(v, dst);
    else *dst = v;
    if (e.dup_src) {
        f4 d = e.dup_a * *(const f4 *)(e.dup_src + (long long)m * e.dup_cs + n);
        if (e.dup_bias) d += *(const f4 *)(e.dup_bias + n);
        d.x = apply_act(d.x, e.act, e.alpha);
        d.y = apply_act(d.y, e.act, e.alpha);
        d.z = apply_act(d.z, e.act, e.alpha);
        d.w = apply_act(d.w, e.act, e.alpha);
        *(f4 *)(a.y + (long long)bidx * a.y_bs + (long long)m * a.ycs + e.dup_off + n) = d;
    }
}

}  // namespace s2v
