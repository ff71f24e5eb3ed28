// The arithmetic between the preprocessing networks (S3FD -> FAN -> 3DMM regressor -> DNet) on the device:
//
//   * fan_landmarks_kernel: get_preds_fromhm's preds_orig (third_part/face_detection/utils.py:163-168): the
//     heatmap points of s2v_fan_peaks through each face's inverse transform matrix, truncated by .int();
//   * face3d_align_kernel: facing.py:110-116 (the landmark fix-up) and align_img's parameters
//     (third_part/face3d/util/preprocess.py:18-43, :147-158, :173-216) for every frame of a clip, with the fit
//     validation of inference._usable_landmarks;
//   * dnet_windows_kernel: the DNet coefficient windows of facing.py:176-187 (futils/inference_utils.py:73-99).
//
// All three are latency-bound glue over a few thousand values: one wave per frame or one small block per
// window, no LDS staging, nothing to tune.  What they owe is the arithmetic stated in include/s2v.h.
#include "common.hpp"

namespace s2v {
namespace {

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------ landmarks
// One thread per (face, point).  v = (m0 x + m1 y) + m2, every step rounded to fp32 on its own.
__global__ __launch_bounds__(256) void fan_landmarks_kernel(const float *__restrict__ preds,
                                                            const float *__restrict__ mats, int faces, int k,
                                                            float *__restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= faces * k) return;
    const float *m = mats + 6 * (e / k);
    const float x = preds[2 * e], y = preds[2 * e + 1];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const float v = __fadd_rn(__fadd_rn(__fmul_rn(m[3 * a], x), __fmul_rn(m[3 * a + 1], y)), m[3 * a + 2]);
        out[2 * e + a] = (float)__float2int_rz(v);
    }
}

// ------------------------------------------------------------------------------ align
constexpr double MAX_DOWNSCALE = 11.5;       // face3d.MAX_DOWNSCALE: s2v_pil_resize_crop's 48-tap limit
constexpr double INT_LIMIT = 2147483648.0;   // 2^31

struct AlignConst {
    double pinv[4][5];
    double target, rescale;
    int default_box[4];
    float default_trans[5];
};

__device__ __forceinline__ bool fits_int(double v) { return v > -INT_LIMIT && v < INT_LIMIT; }   // false for NaN

// POS + resize_n_crop_img's box from five points, all in fp64.  Returns whether s2v_pil_resize_crop can
// take the box (inference._usable_landmarks' rule); box and tr are written only then.
__device__ bool align_fit(const double (*p)[2], const AlignConst &c, int w0, int h0, int *box, float *tr) {
    double kx[4], ky[4];
    for (int r = 0; r < 4; ++r) {
        double ax = 0.0, ay = 0.0;
        for (int j = 0; j < 5; ++j) {
            ax = ax + c.pinv[r][j] * p[j][0];
            ay = ay + c.pinv[r][j] * p[j][1];
        }
        kx[r] = ax;
        ky[r] = ay;
    }
    const double n1 = sqrt((kx[0] * kx[0] + kx[1] * kx[1]) + kx[2] * kx[2]);
    const double n2 = sqrt((ky[0] * ky[0] + ky[1] * ky[1]) + ky[2] * ky[2]);
    const double s = c.rescale / ((n1 + n2) / 2.0);
    const double t0 = kx[3], t1 = ky[3];
    const double wd = (double)w0 * s, hd = (double)h0 * s;
    if (!fits_int(wd) || !fits_int(hd)) return false;
    const int w = (int)wd, h = (int)hd;                  // toward zero
    if (w <= 0 || h <= 0) return false;
    if ((double)w0 / (double)w > MAX_DOWNSCALE || (double)h0 / (double)h > MAX_DOWNSCALE) return false;
    const double ld = ((double)w / 2.0 - c.target / 2.0) + (t0 - (double)w0 / 2.0) * s;
    const double ud = ((double)h / 2.0 - c.target / 2.0) + ((double)h0 / 2.0 - t1) * s;
    if (!fits_int(ld) || !fits_int(ud)) return false;
    box[0] = w;
    box[1] = h;
    box[2] = (int)ld;
    box[3] = (int)ud;
    tr[0] = (float)w0;
    tr[1] = (float)h0;
    tr[2] = (float)s;
    tr[3] = (float)t0;
    tr[4] = (float)t1;
    return true;
}

// One wave64 per frame: the lanes test the 136 values against -1, lane 0 does the fit.
__global__ __launch_bounds__(64) void face3d_align_kernel(const float *__restrict__ lms, int w0, int h0, AlignConst c,
                                                          int *__restrict__ params, float *__restrict__ trans,
                                                          int *__restrict__ status) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const float *lm = lms + (long long)f * 136;
    bool none = true;
    for (int i = lane; i < 136; i += 64) none = none && lm[i] == -1.f;
    const bool no_landmarks = __all(none ? 1 : 0) != 0;
    if (lane != 0) return;
    int box[4];
    float tr[5];
    int st = 1;
    bool ok = false;
    if (!no_landmarks) {
        // frame_landmarks' flip and extract_5p in fp32: points 31, 37, 40, 43, 46, 49, 55 (1-based), the eyes
        // as two-point means, then the order [1, 2, 0, 3, 4]
        const float top = (float)(h0 - 1);
        auto px = [&](int i) { return lm[2 * i]; };
        auto py = [&](int i) { return __fsub_rn(top, lm[2 * i + 1]); };
        auto mean = [](float a, float b) { return __fdiv_rn(__fadd_rn(a, b), 2.f); };
        double p[5][2] = {{(double)mean(px(36), px(39)), (double)mean(py(36), py(39))},
                          {(double)mean(px(42), px(45)), (double)mean(py(42), py(45))},
                          {(double)px(30), (double)py(30)},
                          {(double)px(48), (double)py(48)},
                          {(double)px(54), (double)py(54)}};
        ok = align_fit(p, c, w0, h0, box, tr);
        st = ok ? 0 : 2;
    }
    for (int i = 0; i < 4; ++i) params[4 * f + i] = ok ? box[i] : c.default_box[i];
    for (int i = 0; i < 5; ++i) trans[5 * f + i] = ok ? tr[i] : c.default_trans[i];
    status[f] = st;
}

// ------------------------------------------------------------------------------ windows
constexpr int WIN = 26, ROWS = 73, SEM = 262;

__device__ __forceinline__ int window_column(int r) {
    return r < 64 ? 80 + r : r < 67 ? 224 + (r - 64) : r < 70 ? 254 + (r - 67) : 259 + (r - 70);
}

// One block per window.  The ratio's frame is the first whose 67 expression and angle values compare equal
// to the source's; the source equals itself, so only the frames before it are searched.
__global__ __launch_bounds__(256) void dnet_windows_kernel(const float *__restrict__ sem, int n_frames, int start,
                                                           const float *__restrict__ expression, int one_shot,
                                                           float *__restrict__ out) {
    __shared__ int first;
    const int idx = start + blockIdx.x, tid = threadIdx.x;
    const int src = one_shot ? 0 : idx;
    const float *s = sem + (long long)src * SEM;
    if (tid == 0) first = src;
    __syncthreads();
    for (int j = tid; j < src; j += 256) {
        const float *t = sem + (long long)j * SEM;
        bool same = true;
        for (int k = 0; k < 64 && same; ++k) same = t[80 + k] == s[80 + k];
        for (int k = 0; k < 3 && same; ++k) same = t[224 + k] == s[224 + k];
        if (same) atomicMin(&first, j);
    }
    __syncthreads();
    const float ratio = __fdiv_rn(s[259], sem[(long long)first * SEM + 259]);
    float *o = out + (long long)blockIdx.x * ROWS * WIN;
    for (int e = tid; e < ROWS * WIN; e += 256) {
        const int r = e / WIN, c = e - r * WIN;
        const int f = min(max(idx - 13 + c, 0), n_frames - 1);
        float v = sem[(long long)f * SEM + window_column(r)];
        if (r == 70 && ratio != 0.f) v = __fmul_rn(v, ratio);      // `if crop_norm_ratio:`; NaN is truthy
        if (r < 64 && expression) v = expression[r];
        o[e] = v;
    }
}

}  // namespace
}  // namespace s2v

using namespace s2v;

extern "C" int s2v_fan_landmarks(const float *preds, const float *mats, int faces, int k, float *out,
                                 s2v_stream_t stream) {
    S2V_REQUIRE(preds && mats && out && faces > 0 && k > 0, "fan_landmarks: bad args");
    S2V_REQUIRE((long long)faces * k < (1LL << 28), "fan_landmarks: %d faces of %d points is too many", faces, k);
    fan_landmarks_kernel<<<cdiv((long long)faces * k, 256), 256, 0, (hipStream_t)stream>>>(preds, mats, faces, k, out);
    return check_launch("fan_landmarks");
}

extern "C" int s2v_face3d_align(const float *lms, int n, int w0, int h0, const int *default_box,
                                const float *default_trans, const double *pinv, double target_size,
                                double rescale_factor, int *params, float *trans, int *status, s2v_stream_t stream) {
    S2V_REQUIRE(lms && default_box && default_trans && pinv && params && trans && status && n > 0,
                "face3d_align: bad args");
    S2V_REQUIRE(w0 > 0 && h0 > 0 && w0 < (1 << 24) && h0 < (1 << 24), "face3d_align: %dx%d frames", w0, h0);
    S2V_REQUIRE(target_size > 0 && rescale_factor > 0, "face3d_align: target size %g, rescale factor %g", target_size,
                rescale_factor);
    AlignConst c;
    for (int i = 0; i < 4; ++i) c.default_box[i] = default_box[i];
    for (int i = 0; i < 5; ++i) c.default_trans[i] = default_trans[i];
    for (int i = 0; i < 20; ++i) c.pinv[i / 5][i % 5] = pinv[i];
    c.target = target_size;
    c.rescale = rescale_factor;
    face3d_align_kernel<<<(unsigned)n, 64, 0, (hipStream_t)stream>>>(lms, w0, h0, c, params, trans, status);
    return check_launch("face3d_align");
}

extern "C" int s2v_dnet_windows(const float *semantic, int n_frames, int start, int stop, const float *expression,
                                int one_shot, float *out, s2v_stream_t stream) {
    S2V_REQUIRE(semantic && out && n_frames > 0, "dnet_windows: bad args");
    S2V_REQUIRE(0 <= start && start < stop && stop <= n_frames, "dnet_windows: frames [%d, %d) of %d", start, stop,
                n_frames);
    dnet_windows_kernel<<<(unsigned)(stop - start), 256, 0, (hipStream_t)stream>>>(semantic, n_frames, start, expression,
                                                                                  one_shot ? 1 : 0, out);
    return check_launch("dnet_windows");
}
