// S3FD face detector pieces around the VGG-16 convs (third_part/face_detection/detection/sfd/
// net_s3fd.py, detect.py, bbox.py; api.py:64-79):
//
//   * the batched detector input: uint8 HWC frames -> fp32 NHWC4 minus per-channel means, with the
//     channel flip of FaceAlignment.get_detections_for_batch (images[..., ::-1]) applied first;
//   * L2Norm.forward (net_s3fd.py:16-19) on NHWC maps: a per-pixel reduction over the channel row;
//   * batch_detect's softmax + threshold + prior decode (detect.py:72-92, bbox.batch_decode) over the
//     six fused [conf | loc] head maps of a batch, survivors compacted per image (the NMS over the
//     few survivors stays on the host, as in the reference).
//
// Float expressions are evaluated unfused, in the reference's order.
#include "common.hpp"

#pragma clang fp contract(off)

namespace s2v {
namespace {

unsigned grid_1d(long long total, int per_block = 256) {
    long long b = (total + per_block - 1) / per_block;
    if (b > 65535LL * 32) b = 65535LL * 32;
    return (unsigned)(b < 1 ? 1 : b);
}

// ------------------------------------------------------------------------------ detector input
struct Mean3 {
    float v[3];
};

// imgs = imgs[..., ::-1] (flip) then imgs - (m0, m1, m2) then .float(): uint8 minus an integer-valued
// mean is exact in fp32; channel 3 of NHWC4 is zero
__global__ __launch_bounds__(256) void u8_mean_nhwc4_kernel(const unsigned char *__restrict__ x, long long total,
                                                            Mean3 m, int flip, float *__restrict__ y) {
    for (long long p = blockIdx.x * 256LL + threadIdx.x; p < total; p += (long long)gridDim.x * 256) {
        const unsigned char *s = x + p * 3;
        float4 v;
        v.x = (float)s[flip ? 2 : 0] - m.v[0];
        v.y = (float)s[1] - m.v[1];
        v.z = (float)s[flip ? 0 : 2] - m.v[2];
        v.w = 0.f;
        *(float4 *)(y + p * 4) = v;
    }
}

// ------------------------------------------------------------------------------ L2Norm
// norm = x.pow(2).sum(dim=1).sqrt() + eps; y = x / norm * w: one wavefront per pixel, lane l holds the
// float4 groups l, l + 64, ... of the channel row (V groups per lane, c <= 256 V), the squares are
// summed per lane and across the wave by an xor butterfly (every lane ends with the same sum), and the
// row is scaled from the registers it was loaded into.
template <int V>
__global__ __launch_bounds__(256) void l2norm_nhwc_kernel(const float *__restrict__ x, long long pixels, int c4,
                                                          long long x_cs, const float *__restrict__ w, float eps,
                                                          float *__restrict__ y, long long y_cs) {
    const int lane = threadIdx.x & 63;
    const long long wave = blockIdx.x * 4LL + (threadIdx.x >> 6);
    for (long long p = wave; p < pixels; p += (long long)gridDim.x * 4) {
        const float *row = x + p * x_cs;
        float4 v[V];
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int g = lane + 64 * k;
            v[k] = g < c4 ? *(const float4 *)(row + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
            acc = acc + (v[k].x * v[k].x + v[k].y * v[k].y) + (v[k].z * v[k].z + v[k].w * v[k].w);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
        const float norm = sqrtf(acc) + eps;
        float *out = y + p * y_cs;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int g = lane + 64 * k;
            if (g >= c4) continue;
            const float4 ww = *(const float4 *)(w + 4 * g);
            float4 r;
            r.x = v[k].x / norm * ww.x;
            r.y = v[k].y / norm * ww.y;
            r.z = v[k].z / norm * ww.z;
            r.w = v[k].w / norm * ww.w;
            *(float4 *)(out + 4 * g) = r;
        }
    }
}

// ------------------------------------------------------------------------------ decode
constexpr int S3FD_LEVELS = 6;

struct S3fdLevels {
    const float *head[S3FD_LEVELS];   // fused head output per level: NHWC [n, h, w, cs] with channels
                                      // level 0: [conf (4) | loc (4)], levels 1-5: [conf (2) | loc (4)]
    int h[S3FD_LEVELS], w[S3FD_LEVELS];
    int cs;
    long long first[S3FD_LEVELS + 1];   // first position index of each level (first[6] = positions per image)
};

// one thread per (image, level, row, column); position index = first[level] + row * w + column
__global__ __launch_bounds__(256) void s3fd_decode_kernel(S3fdLevels L, int n, float thresh, float *__restrict__ cand,
                                                          int *__restrict__ count, int max_cand) {
    const long long P = L.first[S3FD_LEVELS];
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < (long long)n * P; e += (long long)gridDim.x * 256) {
        const int b = (int)(e / P);
        const long long q = e - (long long)b * P;
        int lv = 0;
#pragma unroll
        for (int l = 1; l < S3FD_LEVELS; ++l) lv += q >= L.first[l] ? 1 : 0;
        const long long pix = q - L.first[lv];
        const int hi = (int)(pix / L.w[lv]), wi = (int)(pix % L.w[lv]);
        const float *hd = L.head[lv] + ((long long)b * L.h[lv] * L.w[lv] + pix) * L.cs;
        // level 0: max-out background label (net_s3fd.py:124-127)
        float c0, c1;
        const float *lc;
        if (lv == 0) {
            c0 = fmaxf(fmaxf(hd[0], hd[1]), hd[2]);
            c1 = hd[3];
            lc = hd + 4;
        } else {
            c0 = hd[0];
            c1 = hd[1];
            lc = hd + 2;
        }
        // softmax over the two class logits (x - max, exp, * 1 / sum)
        const float mx = fmaxf(c0, c1);
        const float e0 = expf(c0 - mx), e1 = expf(c1 - mx);
        const float score = e1 * (1.f / (e0 + e1));
        if (!(score > thresh)) continue;
        const float stride = (float)(1 << (lv + 2));
        const float pcx = stride / 2.f + (float)wi * stride, pcy = stride / 2.f + (float)hi * stride;
        const float pw = stride * 4.f;
        const float cx = pcx + lc[0] * 0.1f * pw, cy = pcy + lc[1] * 0.1f * pw;
        const float bw = pw * expf(lc[2] * 0.2f), bh = pw * expf(lc[3] * 0.2f);
        const float x1 = cx - bw / 2.f, y1 = cy - bh / 2.f;
        const float x2 = bw + x1, y2 = bh + y1;
        const int slot = atomicAdd(count + b, 1);
        if (slot >= max_cand) continue;
        float *o = cand + ((long long)b * max_cand + slot) * 8;
        o[0] = __int_as_float((int)q);
        o[1] = x1;
        o[2] = y1;
        o[3] = x2;
        o[4] = y2;
        o[5] = score;
        o[6] = 0.f;
        o[7] = 0.f;
    }
}

}  // namespace
}  // namespace s2v

using namespace s2v;

extern "C" int s2v_u8_mean_nhwc4(const unsigned char *x, int n, long long pixels, const float *mean, int flip,
                                 float *y, s2v_stream_t stream) {
    S2V_REQUIRE(x && y && mean && n > 0 && pixels > 0 && (flip == 0 || flip == 1), "u8_mean_nhwc4: bad args");
    S2V_REQUIRE(((uintptr_t)y & 15) == 0, "u8_mean_nhwc4: y must be 16-byte aligned");
    const Mean3 m = {{mean[0], mean[1], mean[2]}};
    const long long total = (long long)n * pixels;
    u8_mean_nhwc4_kernel<<<grid_1d(total), 256, 0, (hipStream_t)stream>>>(x, total, m, flip, y);
    return check_launch("u8_mean_nhwc4");
}

extern "C" int s2v_l2norm_nhwc(const float *x, long long pixels, int c, long long x_cs, const float *weight,
                               float eps, float *y, long long y_cs, s2v_stream_t stream) {
    S2V_REQUIRE(x && y && weight && pixels > 0 && c > 0, "l2norm_nhwc: bad args");
    S2V_REQUIRE(c % 4 == 0 && c <= 1024, "l2norm_nhwc: %d channels (a multiple of 4, at most 1024)", c);
    S2V_REQUIRE(x_cs >= c && y_cs >= c && x_cs % 4 == 0 && y_cs % 4 == 0,
                "l2norm_nhwc: pixel pitches %lld / %lld must be multiples of 4 and >= %d channels", x_cs, y_cs, c);
    S2V_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)weight) & 15) == 0,
                "l2norm_nhwc: x, y and weight must be 16-byte aligned");
    const int c4 = c / 4;
    const unsigned g = grid_1d(pixels, 4);
    hipStream_t s = (hipStream_t)stream;
    if (c4 <= 64) l2norm_nhwc_kernel<1><<<g, 256, 0, s>>>(x, pixels, c4, x_cs, weight, eps, y, y_cs);
    else if (c4 <= 128) l2norm_nhwc_kernel<2><<<g, 256, 0, s>>>(x, pixels, c4, x_cs, weight, eps, y, y_cs);
    else l2norm_nhwc_kernel<4><<<g, 256, 0, s>>>(x, pixels, c4, x_cs, weight, eps, y, y_cs);
    return check_launch("l2norm_nhwc");
}

extern "C" int s2v_s3fd_decode(const float *const *heads, const int *hs, const int *ws, int cs, int n, float thresh,
                               float *cand, int *count, int max_cand, s2v_stream_t stream) {
    S2V_REQUIRE(heads && hs && ws && cand && count && n > 0 && max_cand > 0 && cs >= 8, "s3fd_decode: bad args");
    S3fdLevels L;
    L.cs = cs;
    L.first[0] = 0;
    for (int l = 0; l < S3FD_LEVELS; ++l) {
        S2V_REQUIRE(heads[l] && hs[l] > 0 && ws[l] > 0, "s3fd_decode: level %d missing or empty (%dx%d)", l,
                    heads[l] ? hs[l] : 0, heads[l] ? ws[l] : 0);
        L.head[l] = heads[l];
        L.h[l] = hs[l];
        L.w[l] = ws[l];
        L.first[l + 1] = L.first[l] + (long long)hs[l] * ws[l];
    }
    const long long P = L.first[S3FD_LEVELS];
    S2V_REQUIRE(P < (1LL << 31) && max_cand >= P, "s3fd_decode: max_cand %d < %lld positions per image", max_cand, P);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, sizeof(int) * (size_t)n, st) != hipSuccess) return check_launch("s3fd_decode(memset)");
    s3fd_decode_kernel<<<grid_1d((long long)n * P), 256, 0, st>>>(L, n, thresh, cand, count, max_cand);
    return check_launch("s3fd_decode");
}
