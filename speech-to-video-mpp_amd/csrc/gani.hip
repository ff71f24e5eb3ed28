// GANimation upper-face editing around the SplitGenerator convs (third_part/ganimation_replicate/model/
// ganimation.py:50-53, model_utils.py:474-482) and the --without_rl1 composite (inference.py:269-288):
//
//   * gani_input_kernel: the generator input.  uint8 HWC originals -> F.interpolate(u8 / 255 * 2 - 1, (oh, ow),
//     'bilinear') in channels 0-2 and the image's 17 action units broadcast into channels 3-19 (SplitGenerator's
//     torch.cat([img, sparse_au], 1)), fp32 NHWC with a pixel pitch of 20 floats;
//   * gani_blend_kernel: the two tops' activations on the stacked 4-channel head output (tanh on the colour
//     logits, sigmoid on the mask logit) and GANimationModel.forward's fake = a * src + (1 - a) * color, NCHW;
//   * gani_compose_kernel: cur = F.interpolate(fake / 2 + 0.5, (ph, pw), 'bilinear') (or the originals / 255),
//     mask = (incomplete == 0) and pred * mask + cur * (1 - mask), stored as fp32 or as the truncated uint8 of
//     ``pred.cpu().numpy() * 255``.
//
// torch's bilinear (align_corners=False; UpSampleBilinear2d) restated: scale = (float)in / out; src = scale *
// (dst + 0.5) - 0.5, clamped at 0; i0 = min((int)src, in - 1), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1;
// v = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11), all fp32.  The source coordinate is ONE fused
// multiply-add, as torch's builds evaluate it (CPU and device alike contract that expression): at a coordinate
// near 127 the unfused form lands an ulp (7.6e-6) away, which moves a 3x upsampled pixel by up to 4e-6.  All
// other expressions are evaluated unfused, in the reference's order.
#include "common.hpp"

#pragma clang fp contract(off)

namespace s2v {
namespace {

constexpr int GA_AUS = 17;             // action units per image
constexpr int GA_CS = 3 + GA_AUS;      // channels of the generator input: 20 floats = five float4 per pixel
constexpr int GA_PX = 4;               // compose: pixels per thread
constexpr int GA_TX = 64;              // compose: threads along x (256 pixels per block row)
constexpr int GA_TY = 4;               // compose: rows per block

struct Lerp {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ Lerp ga_lerp(int dst, float scale, int in) {
    float src = fmaf(scale, (float)dst + 0.5f, -0.5f);
    src = src < 0.f ? 0.f : src;
    Lerp r;
    r.i0 = min((int)src, in - 1);
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = fminf(fmaxf(src - (float)r.i0, 0.f), 1.f);
    r.l0 = 1.f - r.l1;
    return r;
}

__device__ __forceinline__ float ga_m11(unsigned char v) { return (float)v / 255.f * 2.f - 1.f; }

// one thread per output pixel
__global__ __launch_bounds__(256) void gani_input_kernel(const unsigned char *__restrict__ x, int h, int w,
                                                         long long xrs, long long xis,
                                                         const float *__restrict__ aus, float *__restrict__ y,
                                                         int oh, int ow, float sy, float sx, long long total) {
    for (long long p = blockIdx.x * 256LL + threadIdx.x; p < total; p += (long long)gridDim.x * 256) {
        const int ox = (int)(p % ow);
        const int oy = (int)((p / ow) % oh);
        const int b = (int)(p / ((long long)ow * oh));
        const Lerp ly = ga_lerp(oy, sy, h), lx = ga_lerp(ox, sx, w);
        const unsigned char *r0 = x + b * xis + ly.i0 * xrs, *r1 = x + b * xis + ly.i1 * xrs;
        float v[GA_CS];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v00 = ga_m11(r0[lx.i0 * 3 + c]), v01 = ga_m11(r0[lx.i1 * 3 + c]);
            const float v10 = ga_m11(r1[lx.i0 * 3 + c]), v11 = ga_m11(r1[lx.i1 * 3 + c]);
            v[c] = ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
        }
        const float *a = aus + (long long)b * GA_AUS;
#pragma unroll
        for (int k = 0; k < GA_AUS; ++k) v[3 + k] = a[k];
        float4 *d = reinterpret_cast<float4 *>(y + p * GA_CS);
#pragma unroll
        for (int q = 0; q < GA_CS / 4; ++q) d[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
}

// one thread per pixel: a float4 of head logits and the first float4 of the input pixel in, seven plane values
// out (consecutive lanes write consecutive floats of a plane)
__global__ __launch_bounds__(256) void gani_blend_kernel(const float *__restrict__ head, long long head_cs,
                                                         const float *__restrict__ in, long long in_cs, int n,
                                                         long long hw, float *__restrict__ color,
                                                         float *__restrict__ mask, float *__restrict__ fake) {
    const long long total = (long long)n * hw;
    for (long long p = blockIdx.x * 256LL + threadIdx.x; p < total; p += (long long)gridDim.x * 256) {
        const long long b = p / hw, q = p - b * hw;
        const float4 lg = *reinterpret_cast<const float4 *>(head + p * head_cs);
        const float4 s = *reinterpret_cast<const float4 *>(in + p * in_cs);
        const float a = 1.f / (1.f + expf(-lg.w));
        const float col[3] = {tanhf(lg.x), tanhf(lg.y), tanhf(lg.z)};
        const float src[3] = {s.x, s.y, s.z};
        mask[p] = a;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long o = (b * 3 + c) * hw + q;
            color[o] = col[c];
            fake[o] = a * src[c] + (1.f - a) * col[c];
        }
    }
}

// Four adjacent pixels of a plane row -> one 16-byte (fp32) or 4-byte (uint8) store when the address allows it,
// element stores otherwise (the ragged row end, rows or bases off the alignment).
template <bool U8>
__device__ __forceinline__ void ga_store(void *plane_row, int x0, int n, const float *v) {
    if (U8) {
        unsigned char *d = (unsigned char *)plane_row + x0;
        unsigned q[GA_PX];
#pragma unroll
        for (int k = 0; k < GA_PX; ++k) q[k] = (unsigned)min(max((int)(v[k] * 255.f), 0), 255);
        if (n == GA_PX && ((unsigned long long)d & 3) == 0) {
            *reinterpret_cast<unsigned *>(d) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            return;
        }
#pragma unroll
        for (int k = 0; k < GA_PX; ++k)
            if (k < n) d[k] = (unsigned char)q[k];
    } else {
        float *d = (float *)plane_row + x0;
        if (n == GA_PX && ((unsigned long long)d & 15) == 0) {
            *reinterpret_cast<float4 *>(d) = make_float4(v[0], v[1], v[2], v[3]);
            return;
        }
#pragma unroll
        for (int k = 0; k < GA_PX; ++k)
            if (k < n) d[k] = v[k];
    }
}

template <bool U8>
__global__ __launch_bounds__(GA_TX *GA_TY) void gani_compose_kernel(
    const float *__restrict__ pred, const unsigned char *__restrict__ orig, long long ors, long long ois,
    const float *__restrict__ fake, int fh, int fw, float sy, float sx, int ph, int pw, void *__restrict__ y) {
    const int b = blockIdx.z;
    const int oy = blockIdx.y * GA_TY + threadIdx.y;
    const int ox = (blockIdx.x * GA_TX + threadIdx.x) * GA_PX;
    if (oy >= ph || ox >= pw) return;
    const int n = min(GA_PX, pw - ox);
    const bool lower = oy >= ph / 2;                   // img_masked[:, img_size // 2:] = 0
    const unsigned char *orow = orig + b * ois + oy * ors + (long long)ox * 3;
    Lerp ly, lx[GA_PX];
    if (fake) {
        ly = ga_lerp(oy, sy, fh);
#pragma unroll
        for (int k = 0; k < GA_PX; ++k) lx[k] = ga_lerp(min(ox + k, pw - 1), sx, fw);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long plane = ((long long)b * 3 + c) * ph * pw + (long long)oy * pw;
        const float *prow = pred + plane + ox;
        const float *f0 = nullptr, *f1 = nullptr;
        if (fake) {
            const float *fp = fake + ((long long)b * 3 + c) * fh * fw;
            f0 = fp + (long long)ly.i0 * fw;
            f1 = fp + (long long)ly.i1 * fw;
        }
        float v[GA_PX];
#pragma unroll
        for (int k = 0; k < GA_PX; ++k) {
            v[k] = 0.f;
            if (k >= n) continue;
            const unsigned char u = orow[k * 3 + c];
            float cur;
            if (fake) {
                const float v00 = f0[lx[k].i0] / 2.f + 0.5f, v01 = f0[lx[k].i1] / 2.f + 0.5f;
                const float v10 = f1[lx[k].i0] / 2.f + 0.5f, v11 = f1[lx[k].i1] / 2.f + 0.5f;
                cur = ly.l0 * (lx[k].l0 * v00 + lx[k].l1 * v01) + ly.l1 * (lx[k].l0 * v10 + lx[k].l1 * v11);
            } else {
                cur = (float)u / 255.f;
            }
            const float pv = prow[k];
            const float pc = pv < 0.f ? 0.f : (pv > 1.f ? 1.f : pv);          // torch.clamp: NaN stays NaN
            const float m = (lower || u == 0) ? 1.f : 0.f;
            v[k] = pc * m + cur * (1.f - m);
        }
        if (U8) ga_store<true>((unsigned char *)y + plane, ox, n, v);
        else ga_store<false>((float *)y + plane, ox, n, v);
    }
}

unsigned ga_grid(long long total) {
    long long b = (total + 255) / 256;
    if (b > 65535LL * 32) b = 65535LL * 32;
    return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace
}  // namespace s2v

using namespace s2v;

extern "C" int s2v_gani_input(const unsigned char *x, int n, int h, int w, long long xrs, long long xis,
                              const float *aus, float *y, int oh, int ow, s2v_stream_t stream) {
    S2V_REQUIRE(x && aus && y && n > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "gani_input: bad args");
    S2V_REQUIRE(xrs >= (long long)w * 3 && (n == 1 || xis >= (long long)h * xrs),
                "gani_input: pitches (%lld, %lld) of %dx%d 3-channel images", xrs, xis, h, w);
    S2V_REQUIRE(((uintptr_t)y & 15) == 0, "gani_input: y must be 16-byte aligned");
    const long long total = (long long)n * oh * ow;
    gani_input_kernel<<<ga_grid(total), 256, 0, (hipStream_t)stream>>>(x, h, w, xrs, xis, aus, y, oh, ow,
                                                                      (float)h / oh, (float)w / ow, total);
    return check_launch("gani_input");
}

extern "C" int s2v_gani_blend(const float *head, long long head_cs, const float *in, long long in_cs, int n, int h,
                              int w, float *color_mask, float *aus_mask, float *fake_img, s2v_stream_t stream) {
    S2V_REQUIRE(head && in && color_mask && aus_mask && fake_img && n > 0 && h > 0 && w > 0, "gani_blend: bad args");
    S2V_REQUIRE(head_cs >= 4 && head_cs % 4 == 0 && in_cs >= 4 && in_cs % 4 == 0,
                "gani_blend: pixel pitches %lld / %lld must be multiples of 4, at least 4", head_cs, in_cs);
    S2V_REQUIRE((((uintptr_t)head | (uintptr_t)in) & 15) == 0, "gani_blend: head and in must be 16-byte aligned");
    gani_blend_kernel<<<ga_grid((long long)n * h * w), 256, 0, (hipStream_t)stream>>>(
        head, head_cs, in, in_cs, n, (long long)h * w, color_mask, aus_mask, fake_img);
    return check_launch("gani_blend");
}

extern "C" int s2v_gani_compose(const float *pred, const unsigned char *orig, long long ors, long long ois,
                                const float *fake, int fh, int fw, int n, int ph, int pw, void *y, int out_u8,
                                s2v_stream_t stream) {
    S2V_REQUIRE(pred && orig && y && n > 0 && ph > 0 && pw > 0 && (out_u8 == 0 || out_u8 == 1),
                "gani_compose: bad args");
    S2V_REQUIRE(!fake || (fh > 0 && fw > 0), "gani_compose: fake_img of %dx%d", fh, fw);
    S2V_REQUIRE(ors >= (long long)pw * 3 && (n == 1 || ois >= (long long)ph * ors),
                "gani_compose: pitches (%lld, %lld) of %dx%d 3-channel originals", ors, ois, ph, pw);
    S2V_REQUIRE(out_u8 || ((uintptr_t)y & 3) == 0, "gani_compose: a float output must be 4-byte aligned");
    S2V_REQUIRE(n <= 65535 && cdiv(ph, GA_TY) <= 65535, "gani_compose: grid too large");
    const dim3 grid(cdiv(pw, GA_TX * GA_PX), cdiv(ph, GA_TY), n), block(GA_TX, GA_TY);
    const float sy = fake ? (float)fh / ph : 1.f, sx = fake ? (float)fw / pw : 1.f;
    if (out_u8)
        gani_compose_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(pred, orig, ors, ois, fake, fh, fw, sy, sx,
                                                                          ph, pw, y);
    else
        gani_compose_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(pred, orig, ors, ois, fake, fh, fw, sy,
                                                                           sx, ph, pw, y);
    return check_launch("gani_compose");
}
