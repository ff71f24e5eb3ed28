// Audio loader: interleaved little-endian PCM -> float32 mono at the target rate, in one launch
// (s2v_audio_load, include/s2v.h): decode, downmix and a polyphase windowed-sinc resampler.
//
//   x[i]   = (sum over the channels of frame i, in order, fp32) / (float)channels     (IEEE division)
//   out[k] = sum_{t = -half+1 .. half} x[floor(k down / up) + t] * table[k mod up][t + half - 1]
//
// One 256-thread workgroup makes a tile of up to 1024 consecutive outputs.  The inputs the tile reaches,
// floor(k0 down / up) - half + 1 .. floor(k1 down / up) + half, are decoded and downmixed once into LDS (zero
// outside the clip); every thread then runs the taps of its outputs k0 + tid + 256 j from LDS against the
// table row of its phase in global memory (rows are 16-byte aligned: one float4 per four taps; the table
// of 44.1 -> 16 kHz, 160 x 376 floats, lives in L2).  Each output is one chain of fmaf from 0.0f, taps
// ascending, so its bits do not depend on the tile size, the launch geometry or any sample beyond its taps.
// All sample and output indices are 64-bit: k down passes 2^31 after 110 s of 44.1 kHz audio.
#include "common.hpp"

namespace s2v {
namespace {

constexpr int AUDIO_THREADS = 256;
constexpr int AUDIO_PER_THREAD = 4;                           // outputs per thread: tiles of up to 1024
constexpr int AUDIO_TILE_MAX = AUDIO_THREADS * AUDIO_PER_THREAD;
constexpr int AUDIO_TILE_MIN = 64;
constexpr long long AUDIO_LDS_FLOATS = 16384;                 // 64 KiB of staged input per workgroup

template <int FMT>
struct Pcm;
template <>
struct Pcm<S2V_PCM_U8> {
    using T = unsigned char;
    static __device__ __forceinline__ float f(T v) { return ((float)v - 128.0f) / 128.0f; }
};
template <>
struct Pcm<S2V_PCM_S16> {
    using T = short;
    static __device__ __forceinline__ float f(T v) { return (float)v / 32768.0f; }
};
template <>
struct Pcm<S2V_PCM_S32> {
    using T = int;
    static __device__ __forceinline__ float f(T v) { return (float)v / 2147483648.0f; }
};
template <>
struct Pcm<S2V_PCM_F32> {
    using T = float;
    static __device__ __forceinline__ float f(T v) { return v; }
};
template <>
struct Pcm<S2V_PCM_F64> {
    using T = double;
    static __device__ __forceinline__ float f(T v) { return (float)v; }
};

// CH samples of one frame in one load (CH * sizeof(T) is 2, 4, 8 or 16 bytes and the frame is aligned to it)
template <typename T, int CH>
struct alignas(sizeof(T) * CH) FrameOf {
    T s[CH];
};

// frame ``g`` decoded and downmixed.  CH > 0: that many channels, the frame in one load; CH == 0: any count
template <int FMT, int CH>
__device__ __forceinline__ float audio_frame(const void *pcm, long long g, int channels) {
    if constexpr (FMT == S2V_PCM_S24) {
        const unsigned char *p = (const unsigned char *)pcm + g * 3 * channels;
        float sum = 0.f;
        for (int c = 0; c < channels; ++c, p += 3) {
            const int v = (int)p[0] | ((int)p[1] << 8) | ((int)(signed char)p[2] << 16);
            const float s = (float)v / 8388608.0f;
            sum = c == 0 ? s : sum + s;
        }
        return sum / (float)channels;
    } else {
        using T = typename Pcm<FMT>::T;
        if constexpr (CH > 0) {
            const FrameOf<T, CH> fr = ((const FrameOf<T, CH> *)pcm)[g];
            float sum = Pcm<FMT>::f(fr.s[0]);
#pragma unroll
            for (int c = 1; c < CH; ++c) sum += Pcm<FMT>::f(fr.s[c]);
            return sum / (float)CH;
        } else {
            const T *p = (const T *)pcm + g * channels;
            float sum = Pcm<FMT>::f(p[0]);
            for (int c = 1; c < channels; ++c) sum += Pcm<FMT>::f(p[c]);
            return sum / (float)channels;
        }
    }
}

// up == down: decode + downmix, one frame per thread
template <int FMT, int CH>
__global__ void __launch_bounds__(AUDIO_THREADS)
audio_decode_kernel(const void *__restrict__ pcm, long long n_frames, int channels, float *__restrict__ out) {
    const long long g = (long long)blockIdx.x * AUDIO_THREADS + threadIdx.x;
    if (g < n_frames) out[g] = audio_frame<FMT, CH>(pcm, g, channels);
}

template <int FMT, int CH>
__global__ void __launch_bounds__(AUDIO_THREADS)
audio_resample_kernel(const void *__restrict__ pcm, long long n_frames, int channels,
                      const float *__restrict__ table, int up, int down, int half, int row_stride, int tile,
                      float *__restrict__ out, long long n_out) {
    extern __shared__ __align__(16) float xs[];
    const int tid = threadIdx.x;
    const long long k0 = (long long)blockIdx.x * tile;
    const long long k1 = (k0 + tile < n_out ? k0 + tile : n_out) - 1;       // the tile's last output
    const long long base0 = k0 * down / up;
    const long long in0 = base0 - half + 1;                                 // the clip index of xs[0]
    const int count = (int)(k1 * down / up - base0) + 2 * half;             // <= the launch's LDS floats
    for (int i = tid; i < count; i += AUDIO_THREADS) {
        const long long g = in0 + i;
        xs[i] = g >= 0 && g < n_frames ? audio_frame<FMT, CH>(pcm, g, channels) : 0.f;
    }
    __syncthreads();

    const int taps = 2 * half;
    int xo[AUDIO_PER_THREAD];                                               // xs index of an output's first tap
    const float *wr[AUDIO_PER_THREAD];
    float acc[AUDIO_PER_THREAD];
    bool live[AUDIO_PER_THREAD];
#pragma unroll
    for (int j = 0; j < AUDIO_PER_THREAD; ++j) {
        const int d = tid + AUDIO_THREADS * j;
        live[j] = d < tile && k0 + d <= k1;
        const long long k = live[j] ? k0 + d : k0;                          // a dead slot reruns output k0
        xo[j] = (int)(k * down / up - base0);
        wr[j] = table + (long long)(k % up) * row_stride;
        acc[j] = 0.f;
    }
    int t = 0;
    for (; t + 4 <= taps; t += 4) {
#pragma unroll
        for (int j = 0; j < AUDIO_PER_THREAD; ++j) {
            const float4 w = *(const float4 *)(wr[j] + t);
            acc[j] = fmaf(xs[xo[j] + t], w.x, acc[j]);
            acc[j] = fmaf(xs[xo[j] + t + 1], w.y, acc[j]);
            acc[j] = fmaf(xs[xo[j] + t + 2], w.z, acc[j]);
            acc[j] = fmaf(xs[xo[j] + t + 3], w.w, acc[j]);
        }
    }
    for (; t < taps; ++t) {
#pragma unroll
        for (int j = 0; j < AUDIO_PER_THREAD; ++j) acc[j] = fmaf(xs[xo[j] + t], wr[j][t], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < AUDIO_PER_THREAD; ++j)
        if (live[j]) out[k0 + tid + AUDIO_THREADS * j] = acc[j];
}

// LDS floats a tile of ``tile`` outputs needs at most: floor(k1 down/up) - floor(k0 down/up) <= ceil((tile-1) down/up)
inline long long audio_tile_floats(long long tile, int up, int down, int half) {
    return ((tile - 1) * down + up - 1) / up + 2LL * half;
}

template <int FMT, int CH>
int audio_launch(const void *pcm, long long n_frames, int channels, const float *table, int up, int down, int half,
                 int row_stride, float *out, long long n_out, s2v_stream_t stream) {
    if (up == down) {
        const long long blocks = (n_frames + AUDIO_THREADS - 1) / AUDIO_THREADS;
        S2V_REQUIRE(blocks < 2147483647LL, "audio_load: too long");
        audio_decode_kernel<FMT, CH><<<(unsigned)blocks, AUDIO_THREADS, 0, (hipStream_t)stream>>>(pcm, n_frames,
                                                                                                 channels, out);
        return check_launch("audio_load");
    }
    int tile = AUDIO_TILE_MAX;
    while (tile > AUDIO_TILE_MIN && audio_tile_floats(tile, up, down, half) > AUDIO_LDS_FLOATS) tile /= 2;
    const long long floats = audio_tile_floats(tile, up, down, half);
    S2V_REQUIRE(floats <= AUDIO_LDS_FLOATS, "audio_load: %d taps at %d/%d do not fit the 64 KiB input tile",
                2 * half, down, up);
    const long long blocks = (n_out + tile - 1) / tile;
    S2V_REQUIRE(blocks < 2147483647LL, "audio_load: too long");
    audio_resample_kernel<FMT, CH><<<(unsigned)blocks, AUDIO_THREADS, (size_t)floats * sizeof(float),
                                     (hipStream_t)stream>>>(pcm, n_frames, channels, table, up, down, half,
                                                            row_stride, tile, out, n_out);
    return check_launch("audio_load");
}

template <int FMT>
int audio_dispatch(const void *pcm, long long n_frames, int channels, const float *table, int up, int down, int half,
                   int row_stride, float *out, long long n_out, s2v_stream_t stream) {
    // mono and stereo of the aligned formats take a frame per load
    if constexpr (FMT != S2V_PCM_S24) {
        constexpr size_t sz = sizeof(typename Pcm<FMT>::T);
        if (channels == 1)
            return audio_launch<FMT, 1>(pcm, n_frames, channels, table, up, down, half, row_stride, out, n_out, stream);
        if (channels == 2 && (uintptr_t)pcm % (2 * sz) == 0)
            return audio_launch<FMT, 2>(pcm, n_frames, channels, table, up, down, half, row_stride, out, n_out, stream);
    }
    return audio_launch<FMT, 0>(pcm, n_frames, channels, table, up, down, half, row_stride, out, n_out, stream);
}

}  // namespace
}  // namespace s2v

using namespace s2v;

extern "C" int s2v_audio_load(const void *pcm, long long n_frames, int channels, int format, const float *table,
                              int up, int down, int half, int row_stride, float *out, long long n_out,
                              s2v_stream_t stream) {
    S2V_REQUIRE(n_frames >= 0 && n_out >= 0, "audio_load: negative length");
    S2V_REQUIRE(n_frames == 0 || (pcm && out), "audio_load: null pointer");
    S2V_REQUIRE(channels >= 1, "audio_load: channels must be >= 1 (got %d)", channels);
    S2V_REQUIRE(format >= S2V_PCM_U8 && format <= S2V_PCM_F64, "audio_load: unknown sample format %d", format);
    S2V_REQUIRE(up >= 1 && down >= 1, "audio_load: up and down must be >= 1 (got %d, %d)", up, down);
    S2V_REQUIRE(n_frames <= (1LL << 62) / up / down, "audio_load: too long");
    if (up != down) {
        S2V_REQUIRE(table, "audio_load: null table with up != down");
        S2V_REQUIRE(half >= 1, "audio_load: half must be >= 1 (got %d)", half);
        S2V_REQUIRE(half <= (1 << 24), "audio_load: half too large (%d)", half);
        S2V_REQUIRE(row_stride >= 2 * half, "audio_load: row_stride %d < 2 half = %d", row_stride, 2 * half);
        S2V_REQUIRE(row_stride % 4 == 0 && ((uintptr_t)table & 15) == 0,
                    "audio_load: table rows must be 16-byte aligned (row_stride a multiple of 4)");
    }
    const long long want = up == down ? n_frames : (n_frames * up + down - 1) / down;
    S2V_REQUIRE(n_out == want, "audio_load: n_out must be ceil(n_frames up / down) = %lld (got %lld)", want, n_out);
    if (n_frames == 0) return S2V_OK;
    static const int kBytes[] = {1, 2, 1, 4, 4, 8};             // alignment of a sample (S24: bytes)
    S2V_REQUIRE((uintptr_t)pcm % kBytes[format] == 0, "audio_load: pcm must be aligned to its sample size");
    S2V_REQUIRE(((uintptr_t)out & 3) == 0, "audio_load: out must be 4-byte aligned");
    switch (format) {
        case S2V_PCM_U8:
            return audio_dispatch<S2V_PCM_U8>(pcm, n_frames, channels, table, up, down, half, row_stride, out, n_out, stream);
        case S2V_PCM_S16:
            return audio_dispatch<S2V_PCM_S16>(pcm, n_frames, channels, table, up, down, half, row_stride, out, n_out, stream);
        case S2V_PCM_S24:
            return audio_dispatch<S2V_PCM_S24>(pcm, n_frames, channels, table, up, down, half, row_stride, out, n_out, stream);
        case S2V_PCM_S32:
            return audio_dispatch<S2V_PCM_S32>(pcm, n_frames, channels, table, up, down, half, row_stride, out, n_out, stream);
        case S2V_PCM_F32:
            return audio_dispatch<S2V_PCM_F32>(pcm, n_frames, channels, table, up, down, half, row_stride, out, n_out, stream);
        default:
            return audio_dispatch<S2V_PCM_F64>(pcm, n_frames, channels, table, up, down, half, row_stride, out, n_out, stream);
    }
}
