// The STIT reference stitch of datagen (inference.py:341-367; futils/alignment_stit.py): the FFHQ-style
// rotated square around eyes and mouth is resampled out of the stabilised frame (crop_image, :68-114) and
// pasted back with the inverse perspective transform over the original crop (paste_image, :14-18).
//
//  * pil_transform_quad_kernel: Pillow's Image.transform(size, QUAD, data, BILINEAR) out of a sub-rectangle
//    (crop_image's crop box) of every frame.
//  * pil_perspective_paste_kernel: paste_image in one pass: the RGBA PERSPECTIVE + BILINEAR transform of the
//    crop (through Pillow's premultiplied RGBa round trip) and the masked paste over the target, RGB out.
//
// Pillow's arithmetic (libImaging/Geometry.c, Paste.c, Convert.c) restated:
//    the transform is evaluated at the pixel centre (x + 0.5, y + 0.5) in double, without FMA;
//    a sample outside [0, xsize) x [0, ysize) leaves the output pixel 0 (all bands, alpha included);
//    otherwise xin -= 0.5, x = floor(xin), dx = xin - x, the two columns are clamp(x), clamp(x + 1), the rows
//    clamp(y) and y + 1 when it exists (else the first row's value again);
//    v = a + (b - a) * d in double, three times, then (UINT8)v: truncation;
//    RGBA -> RGBa premultiplies with MULDIV255, RGBa -> RGBA divides (255 * v) / alpha clipped to 255 unless
//    alpha is 0 or 255; paste(mask) is BLEND8 = DIV255(dst * (255 - alpha) + src * alpha) per band.
// Both kernels give each thread four adjacent pixels of a row, so that a 3-byte-pixel row is written as
// three dwords per thread (12 contiguous bytes, consecutive threads contiguous) instead of twelve byte
// stores; rows or buffers that are not 4-byte aligned, and the ragged end of a row, take byte stores.
#include "common.hpp"

namespace s2v {

#pragma clang fp contract(off)

constexpr int ST_PX = 4;          // pixels per thread
constexpr int ST_TX = 64;         // threads along x: 256 pixels per block row
constexpr int ST_TY = 4;          // rows per block

__device__ __forceinline__ int st_muldiv255(int a, int b) {
    const int t = a * b + 128;
    return ((t >> 8) + t) >> 8;
}

// One BILINEAR sample of a C-band uint8 image (w x h, row stride rs bytes) at (xin, yin) -> o[0..C) (o[3] =
// 255 for C == 3).  PREMUL: the RGB bands of every tap are premultiplied by the tap's alpha first.  false:
// outside the image (o untouched).
template <int C, bool PREMUL>
__device__ __forceinline__ bool st_bilinear(const unsigned char *img, long long rs, int w, int h, double xin,
                                            double yin, int *o) {
    if (!(xin >= 0.0 && xin < (double)w && yin >= 0.0 && yin < (double)h)) return false;
    xin -= 0.5;
    yin -= 0.5;
    const int x = (int)floor(xin), y = (int)floor(yin);       // >= -1
    const double dx = xin - x, dy = yin - y;
    const int x0 = (x < 0 ? 0 : x) * C, x1 = (x + 1 > w - 1 ? w - 1 : x + 1) * C;
    const unsigned char *r0 = img + (long long)(y < 0 ? 0 : y) * rs;
    const bool two = y + 1 < h;
    const unsigned char *r1 = img + (long long)(two ? y + 1 : 0) * rs;
    int a00 = 255, a01 = 255, a10 = 255, a11 = 255;
    if (C == 4 && PREMUL) {
        a00 = r0[x0 + 3];
        a01 = r0[x1 + 3];
        a10 = r1[x0 + 3];
        a11 = r1[x1 + 3];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        int p00 = r0[x0 + c], p01 = r0[x1 + c];
        if (C == 4 && PREMUL && c < 3) {
            p00 = st_muldiv255(p00, a00);
            p01 = st_muldiv255(p01, a01);
        }
        double v1 = (double)p00 + ((double)p01 - (double)p00) * dx;
        double v2 = v1;
        if (two) {
            int p10 = r1[x0 + c], p11 = r1[x1 + c];
            if (C == 4 && PREMUL && c < 3) {
                p10 = st_muldiv255(p10, a10);
                p11 = st_muldiv255(p11, a11);
            }
            v2 = (double)p10 + ((double)p11 - (double)p10) * dx;
        }
        o[c] = (int)(v1 + (v2 - v1) * dy) & 255;
    }
    if (C == 3) o[3] = 255;
    return true;
}

// px[k][0..C) of the thread's n (<= 4) pixels starting at column x0 of row ``row`` (C bytes per pixel).
template <int C>
__device__ __forceinline__ void st_store(unsigned char *row, int x0, int n, bool aligned, const int (*px)[4]) {
    unsigned char *d = row + (long long)x0 * C;
    if (aligned && n == ST_PX) {
        unsigned b[ST_PX * C];
#pragma unroll
        for (int k = 0; k < ST_PX; ++k)
#pragma unroll
            for (int c = 0; c < C; ++c) b[k * C + c] = (unsigned)px[k][c];
        unsigned *d4 = reinterpret_cast<unsigned *>(d);
#pragma unroll
        for (int i = 0; i < C; ++i)
            d4[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | (b[4 * i + 3] << 24);
        return;
    }
#pragma unroll
    for (int k = 0; k < ST_PX; ++k)
        if (k < n) {
#pragma unroll
            for (int c = 0; c < C; ++c) d[k * C + c] = (unsigned char)px[k][c];
        }
}

// table[b] = (a0..a7, left, top, width, height): the QUAD coefficients as Image.__transformer forms them,
// relative to the crop box, and the crop box inside the frame.
template <int C>
__global__ __launch_bounds__(ST_TX *ST_TY) void pil_transform_quad_kernel(
    const unsigned char *__restrict__ x, int h, int w, long long xrs, long long xis,
    const double *__restrict__ table, unsigned char *__restrict__ y, int oh, int ow, long long yrs, long long yis,
    int aligned) {
    const int b = blockIdx.z;
    const int oy = blockIdx.y * ST_TY + threadIdx.y;
    const int ox = (blockIdx.x * ST_TX + threadIdx.x) * ST_PX;
    if (oy >= oh || ox >= ow) return;
    const double *t = table + 12 * b;
    // the crop box, clamped into the frame whatever the table holds
    int left = (int)t[8], top = (int)t[9], bw = (int)t[10], bh = (int)t[11];
    left = min(max(left, 0), w - 1);
    top = min(max(top, 0), h - 1);
    bw = min(max(bw, 1), w - left);
    bh = min(max(bh, 1), h - top);
    const unsigned char *img = x + b * xis + top * xrs + (long long)left * C;
    const double a0 = t[0], a1 = t[1], a2 = t[2], a3 = t[3], a4 = t[4], a5 = t[5], a6 = t[6], a7 = t[7];
    const double yc = oy + 0.5;
    const int n = min(ST_PX, ow - ox);
    int px[ST_PX][4];
#pragma unroll
    for (int k = 0; k < ST_PX; ++k) {               // unrolled: px stays in registers
        if (k >= n) continue;
        const double xc = (ox + k) + 0.5;
        const double xin = a0 + a1 * xc + a2 * yc + a3 * xc * yc;
        const double yin = a4 + a5 * xc + a6 * yc + a7 * xc * yc;
        px[k][0] = px[k][1] = px[k][2] = px[k][3] = 0;
        st_bilinear<C, false>(img, xrs, bw, bh, xin, yin, px[k]);
        if (C == 3) px[k][3] = 0;
    }
    st_store<C>(y + b * yis + oy * yrs, ox, n, aligned != 0, px);
}

// coeffs[b] = the eight PERSPECTIVE coefficients (target pixel centre -> crop coordinates).
template <int CC, int TC, int YC>
__global__ __launch_bounds__(ST_TX *ST_TY) void pil_perspective_paste_kernel(
    const unsigned char *__restrict__ crop, int sh, int sw, long long crs, long long cis,
    const double *__restrict__ coeffs, const unsigned char *target, int h, int w, long long trs, long long tis,
    unsigned char *y, long long yrs, long long yis, int aligned) {
    const int b = blockIdx.z;
    const int oy = blockIdx.y * ST_TY + threadIdx.y;
    const int ox = (blockIdx.x * ST_TX + threadIdx.x) * ST_PX;
    if (oy >= h || ox >= w) return;
    const double *a = coeffs + 8 * b;
    const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7];
    const unsigned char *img = crop + b * cis;
    const unsigned char *trow = target + b * tis + oy * trs + (long long)ox * TC;
    const double yc = oy + 0.5;
    const int n = min(ST_PX, w - ox);
    int px[ST_PX][4];
#pragma unroll
    for (int k = 0; k < ST_PX; ++k) {               // unrolled; every read of the target before the first store
        if (k >= n) continue;
        const double xc = (ox + k) + 0.5;
        const double den = a6 * xc + a7 * yc + 1;
        const double xin = (a0 * xc + a1 * yc + a2) / den;
        const double yin = (a3 * xc + a4 * yc + a5) / den;
        int s[4] = {0, 0, 0, 0};
        st_bilinear<CC, true>(img, crs, sw, sh, xin, yin, s);
        const int al = s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int v = s[c];
            if (al != 255 && al != 0) v = min((255 * v) / al, 255);          // RGBa -> RGBA
            const int t = trow[k * TC + c] * (255 - al) + v * al + 128;       // BLEND8
            px[k][c] = ((t >> 8) + t) >> 8;
        }
        px[k][3] = 255;
    }
    st_store<YC>(y + b * yis + oy * yrs, ox, n, aligned != 0, px);
}

static bool st_aligned(const void *p, long long rs, long long is) {
    return ((unsigned long long)p % 4 == 0) && rs % 4 == 0 && is % 4 == 0;
}

// Do the byte ranges of two batches of images ([n][h][w * c bytes], row stride rs, image stride is) overlap?
static bool st_overlap(const void *a, int an, int ah, long long aw, long long ars, long long ais, const void *b,
                       int bn, int bh, long long bw, long long brs, long long bis) {
    const unsigned long long a0 = (unsigned long long)a, b0 = (unsigned long long)b;
    const unsigned long long a1 = a0 + (an - 1) * ais + (ah - 1) * ars + aw;
    const unsigned long long b1 = b0 + (bn - 1) * bis + (bh - 1) * brs + bw;
    return a0 < b1 && b0 < a1;
}

}  // namespace s2v

using namespace s2v;

extern "C" int s2v_pil_transform_quad(const unsigned char *x, int n, int h, int w, int c, long long xrs, long long xis,
                                      const double *table, unsigned char *y, int oh, int ow, long long yrs,
                                      long long yis, s2v_stream_t stream) {
    S2V_REQUIRE(x && table && y && n > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "pil_transform_quad: bad args");
    S2V_REQUIRE(c == 3 || c == 4, "pil_transform_quad: 3 or 4 channels, got %d", c);
    S2V_REQUIRE(xrs >= (long long)w * c && (n == 1 || xis >= (long long)h * xrs) && yrs >= (long long)ow * c &&
                    (n == 1 || yis >= (long long)oh * yrs),
                "pil_transform_quad: strides x (%lld, %lld) y (%lld, %lld)", xrs, xis, yrs, yis);
    S2V_REQUIRE(!st_overlap(x, n, h, (long long)w * c, xrs, xis, y, n, oh, (long long)ow * c, yrs, yis),
                "pil_transform_quad: the output overlaps the frames");
    S2V_REQUIRE(n <= 65535 && cdiv(oh, ST_TY) <= 65535, "pil_transform_quad: grid too large");
    const dim3 grid(cdiv(ow, ST_TX * ST_PX), cdiv(oh, ST_TY), n), block(ST_TX, ST_TY);
    const int al = st_aligned(y, yrs, yis);
    if (c == 3)
        pil_transform_quad_kernel<3><<<grid, block, 0, (hipStream_t)stream>>>(x, h, w, xrs, xis, table, y, oh, ow,
                                                                             yrs, yis, al);
    else
        pil_transform_quad_kernel<4><<<grid, block, 0, (hipStream_t)stream>>>(x, h, w, xrs, xis, table, y, oh, ow,
                                                                             yrs, yis, al);
    return check_launch("pil_transform_quad");
}

#define ST_PASTE(CC, TC, YC)                                                                                   \
    pil_perspective_paste_kernel<CC, TC, YC><<<grid, block, 0, (hipStream_t)stream>>>(                         \
        crop, sh, sw, crs, cis, coeffs, target, h, w, trs, tis, y, yrs, yis, al)

extern "C" int s2v_pil_perspective_paste(const unsigned char *crop, int n, int sh, int sw, int cc, long long crs,
                                         long long cis, const double *coeffs, const unsigned char *target, int h,
                                         int w, int tc, long long trs, long long tis, unsigned char *y, int yc,
                                         long long yrs, long long yis, s2v_stream_t stream) {
    S2V_REQUIRE(crop && coeffs && target && y && n > 0 && sh > 0 && sw > 0 && h > 0 && w > 0,
                "pil_perspective_paste: bad args");
    S2V_REQUIRE((cc == 3 || cc == 4) && (tc == 3 || tc == 4) && (yc == 3 || yc == 4),
                "pil_perspective_paste: 3 or 4 channels, got crop %d target %d out %d", cc, tc, yc);
    S2V_REQUIRE(crs >= (long long)sw * cc && (n == 1 || cis >= (long long)sh * crs) && trs >= (long long)w * tc &&
                    (n == 1 || tis >= (long long)h * trs) && yrs >= (long long)w * yc &&
                    (n == 1 || yis >= (long long)h * yrs),
                "pil_perspective_paste: strides crop (%lld, %lld) target (%lld, %lld) y (%lld, %lld)", crs, cis, trs,
                tis, yrs, yis);
    // every thread reads its own target pixels before it stores them, so the same buffer in the same layout is
    // safe; any other overlap lets one thread's store reach another thread's read
    S2V_REQUIRE(target == y ? (tc == yc && trs == yrs && tis == yis)
                            : !st_overlap(target, n, h, (long long)w * tc, trs, tis, y, n, h, (long long)w * yc, yrs, yis),
                "pil_perspective_paste: target and output overlap (in place needs the same pointer and layout)");
    S2V_REQUIRE(!st_overlap(crop, n, sh, (long long)sw * cc, crs, cis, y, n, h, (long long)w * yc, yrs, yis),
                "pil_perspective_paste: the output overlaps the crops");
    S2V_REQUIRE(n <= 65535 && cdiv(h, ST_TY) <= 65535, "pil_perspective_paste: grid too large");
    const dim3 grid(cdiv(w, ST_TX * ST_PX), cdiv(h, ST_TY), n), block(ST_TX, ST_TY);
    const int al = st_aligned(y, yrs, yis);
    const int key = (cc == 4) * 4 + (tc == 4) * 2 + (yc == 4);
    switch (key) {
        case 0: ST_PASTE(3, 3, 3); break;
        case 1: ST_PASTE(3, 3, 4); break;
        case 2: ST_PASTE(3, 4, 3); break;
        case 3: ST_PASTE(3, 4, 4); break;
        case 4: ST_PASTE(4, 3, 3); break;
        case 5: ST_PASTE(4, 3, 4); break;
        case 6: ST_PASTE(4, 4, 3); break;
        default: ST_PASTE(4, 4, 4); break;
    }
    return check_launch("pil_perspective_paste");
}
