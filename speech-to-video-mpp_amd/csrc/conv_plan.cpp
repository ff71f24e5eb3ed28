// The convolution planner: tile tables, route predicates, validate and make_plan (conv_plan.hpp).
// Host only: no HIP headers, no kernels; needs include/s2v.h and a device_cus() / set_error() to link.
#include "conv_plan.hpp"

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace s2v {

// ------------------------------------------------------------------ knobs
// planner knobs (s2v_tune; defaults, or S2V_HALO_MIN_BLOCKS / S2V_GLDS_TILE / ... from the environment)
static const struct { const char *env; long long def; } kKnobs[S2V_TUNE_COUNT] = {   // indexed by S2V_TUNE_*
    {"S2V_HALO_MIN_BLOCKS", 0}, {"S2V_GLDS_TILE", -1}, {"S2V_SMALLK_TILE", 1}, {"S2V_X3_RATE_512", 0},
    {"S2V_IN_FUSED", 576},      // max plane pixels of the one-launch InstanceNorm
    {"S2V_RESIZE_UP2", 1}};
static_assert(S2V_TUNE_HALO_MIN_BLOCKS == 0 && S2V_TUNE_GLDS_TILE == 1 && S2V_TUNE_SMALLK_TILE == 2 &&
              S2V_TUNE_X3_RATE_512 == 3 && S2V_TUNE_IN_FUSED == 4 && S2V_TUNE_RESIZE_UP2 == 5, "kKnobs order");
static long long g_tune[S2V_TUNE_COUNT];
static bool g_tune_init = false;
long long tune_get(int key) {
    for (int i = 0; i < S2V_TUNE_COUNT && !g_tune_init; ++i) {   // read once
        const char *e = getenv(kKnobs[i].env);
        g_tune[i] = e ? atoll(e) : kKnobs[i].def;
    }
    g_tune_init = true;
    return g_tune[key];
}

long long tune_set(int key, long long value) {
    const long long prev = tune_get(key);
    g_tune[key] = value;
    return prev;
}

// S2V_HEAD_X3=0: the fp32 VALU kernels instead of conv_head_x3
static bool head_x3_on() {
    static const int on = [] { const char *e = getenv("S2V_HEAD_X3"); return e ? atoi(e) : 1; }();
    return on != 0;
}
// S2V_K4=0: the split-precision tiles / conv_smallk4 instead of conv_k4_mfma
static bool k4_on() {
    static const int on = [] { const char *e = getenv("S2V_K4"); return e ? atoi(e) : 1; }();
    return on != 0;
}
// candidate tiles of a conv group (kX3Tiles indices; S2V_GROUP_TILES overrides, e.g. "0,6,4,3,1")
static const std::vector<int> &group_tiles() {
    static const std::vector<int> cands = [] {
        std::vector<int> v;
        const char *e = getenv("S2V_GROUP_TILES");
        if (e && *e) {
            for (const char *q = e; *q;) {
                const int t = atoi(q);
                if (t == 0 || t == 1 || t == 3 || t == 4 || t == 6) v.push_back(t);
                while (*q && *q != ',') ++q;
                if (*q == ',') ++q;
            }
        }
        if (v.empty()) v = {4, 3, 1};
        return v;
    }();
    return cands;
}

// CUs the planner fills (split-K factors, tile choice): the device's
static int plan_cus() { return device_cus() > 0 ? device_cus() : 256; }

// ------------------------------------------------------------------ tile tables
static const TileCfg kTiles[] = {
    {128, 128, 2, 4, 1, 2}, {128, 64, 2, 4, 1, 2}, {64, 128, 2, 4, 1, 2}, {64, 64, 2, 4, 1, 2}, {256, 32, 4, 4, 1, 2},
    {128, 32, 4, 4, 1, 2}};
constexpr int kNumTiles = sizeof(kTiles) / sizeof(kTiles[0]);
// split-fp32 (S2V_PREC_BF16X3 / F16X3) configurations, conv_x3_impl.hpp launch_conv_x3, with the sustained
// throughput each reaches on a full chip (TFLOP/s fp32-equivalent, MI355X, tools/conv_micro.py r01)
// and resident blocks per CU (LDS / waves) for the planner's cost model
// (512x128: 360, set end to end on MI355X r03 — lipsync 29.11 -> 28.35 ms, its 400^2 N = 128 StyleConvs;
// 420 also displaces the 256x256 tile on N = 256 layers: 28.80 ms)
struct X3Cfg {
    TileCfg t;
    float tflops;
    int bpc;
    int kind = 0;    // 1 / 2: conv_x3_nar (register-direct A / A and B fragments), 3 / 4 / 5: conv_x3_halo
};
static const X3Cfg kX3Tiles[] = {
    {{256, 256, 2, 8, 1, 1}, 400.f, 1}, {{128, 128, 2, 8, 1, 1}, 330.f, 2}, {{64, 128, 2, 8, 1, 1}, 260.f, 3},
    {{128, 64, 2, 4, 1, 1}, 290.f, 3},  {{64, 64, 2, 4, 1, 1}, 265.f, 4},   {{128, 32, 4, 4, 1, 1}, 235.f, 4},
    {{256, 128, 4, 8, 1, 1}, 335.f, 1}, {{256, 64, 8, 8, 1, 1}, 300.f, 2},  {{512, 128, 4, 8, 1, 1}, 360.f, 1},
    // narrow-N tiles with 64-row waves (r04, tools/r04_nsweep.sh on MI355X, graph-timed 3x3 64-channel
    // convs): 4x512^2 128 -> 64 199 (256x64 8-wave) -> 225 (512x64) / 233 (256x64 4-wave) TFLOP/s,
    // 16x256^2 64 -> 64 156 -> 171 / 183; at 96^2 and below 128x64 stays ahead (more blocks).  The
    // rates keep that order in the planner's model.  256x32 (4-wave): no faster than 128x32, forced-only.
    {{512, 64, 8, 8, 1, 1}, 335.f, 1},  {{256, 64, 4, 4, 1, 1}, 350.f, 2},  {{256, 32, 4, 4, 1, 1}, 0.f, 2},
    // deep-stage 4-wave tiles (r05): 2 or 4 K-slices per LDS stage, so a latency-bound small-grid conv (LNet's
    // 12^2 - 48^2 layers: one block per CU, K loops of 6 - 72 slices) waits on half / a quarter as many
    // load round trips; one block per CU by LDS.  Forced-only until measured (tools/lnet_convs.py --tiles)
    {{64, 64, 2, 4, 4, 1}, 0.f, 1},     {{128, 64, 2, 4, 2, 1}, 0.f, 1},   {{128, 32, 4, 4, 2, 1}, 0.f, 1},
    // 256 x 64 with A fragments loaded by each lane straight into registers, B alone through LDS
    // (conv_x3_nar.hip): direct zero-padded convs, cin % 32 == 0, no pooled epilogue, 2^31-byte offsets
    {{256, 64, 4, 4, 1, 1}, 0.f, 2, 1},
    // ... with the B fragments loaded by every wave into registers too: no LDS, no barrier per slice
    {{256, 64, 4, 4, 1, 1}, 0.f, 2, 2},
    // 4 x 64 output patches, 64 channels, the 6 x 66 input halo per channel slice staged once
    // (conv_x3_halo.hip): 3x3 stride-1 zero-padded convs (ragged images: partly empty last patches)
    {{256, 64, 4, 4, 1, 1}, 0.f, 2, 3},
    // ... 8 x 64 patches, one 512-thread block per CU (oh % 8 == 0)
    {{512, 64, 8, 8, 1, 1}, 0.f, 1, 4},
    // ... 4 x 64 patches x 128 output channels (two 64-channel wave columns), one 512-thread block per CU
    {{256, 128, 4, 8, 1, 1}, 0.f, 1, 5}};
constexpr int kNumX3 = sizeof(kX3Tiles) / sizeof(kX3Tiles[0]);

// LDS-DMA kernels (x_split inputs): 256 x BN tiles, BN = 256 when the weight rows allow, else 128
struct GldsCfg {
    int bm, bn, wm, nst;
};
static const GldsCfg kGlds[] = {{256, 256, 2, 2}, {256, 128, 4, 3}, {512, 128, 4, 2}};

// ------------------------------------------------------------------ predicates
static int batch_of(const s2v_conv_params *p) { return p->batch > 0 ? p->batch : 1; }

// blocks of the launch on BM x BN tiles, before split-K
static long long tile_blocks(const Plan &pl, const TileCfg &t) {
    return (long long)cdiv(pl.M, t.bm) * cdiv(pl.cout, t.bn) * pl.batch;
}

// 16-byte epilogue stores are possible (store_epilogue4's vec): aligned rows and per-channel vectors
int epi_vec4(const s2v_conv_params *p) {
    return p->cout % 4 == 0 && p->ycs % 4 == 0 && ((uintptr_t)p->y % 16) == 0 && p->y_bs % 4 == 0 &&
           (!p->res || (p->res_cs % 4 == 0 && ((uintptr_t)p->res % 16) == 0 && p->res_bs % 4 == 0)) &&
           (!p->scale || ((uintptr_t)p->scale % 16) == 0) && (!p->shift || ((uintptr_t)p->shift % 16) == 0) &&
           (!p->post_mul || (p->post_cs % 4 == 0 && p->post_c0 % 4 == 0 && ((uintptr_t)p->post_mul % 16) == 0 &&
                             ((uintptr_t)p->post_add % 16) == 0)) &&
           (!p->dup_src || (p->dup_cs % 4 == 0 && p->dup_off % 4 == 0 && ((uintptr_t)p->dup_src % 16) == 0 &&
                            (!p->dup_bias || ((uintptr_t)p->dup_bias % 16) == 0)));
}

// 16-byte input loads: 4k channels, aligned rows (and in_scale rows)
static bool vec4_input(const s2v_conv_params *p) {
    return (p->cin % 4 == 0) && (p->xcs % 4 == 0) && (((uintptr_t)p->x % 16) == 0) && (p->x_bs % 4 == 0) &&
           (!p->in_scale || (p->in_scale_ns % 4 == 0 && ((uintptr_t)p->in_scale % 16) == 0));
}

static bool use_direct(const s2v_conv_params *p) { return p->cout <= 4 && !p->b_kn; }

// A plain stride-1 square-filter head: Cout <= 4, direct input, zero or reflect padding (pad < filter),
// no prologue scaling, one shared filter, 16-byte aligned rows.
static bool plain_head(const s2v_conv_params *p) {
    return p->cout <= 4 && p->kh == p->kw && p->in_mode == S2V_IN_DIRECT && p->sh == 1 && p->sw == 1 && p->dh == 1 &&
           p->dw == 1 && !p->in_scale && !p->pre_act && !p->w_bs && batch_of(p) == 1 && !p->b_kn && p->out_step <= 1 &&
           p->ph < p->kh && p->pw < p->kw && p->xcs % 4 == 0 && ((uintptr_t)p->x % 16) == 0 &&
           !(p->pad_mode == S2V_PAD_REFLECT && (p->ph >= p->h || p->pw >= p->w));
}

// The fp32 halo kernel serves plain 3x3 / 5x5 / 7x7 heads over 4k channels
static int halo_ks(const s2v_conv_params *p) {
    if (!plain_head(p) || (p->kh != 3 && p->kh != 5 && p->kh != 7) || p->cin % 4) return 0;
    // 8 x 128 output tiles: on small images (LNet's 96^2 RGB head, DNet's 64^2 flow head) too few
    // blocks cover the chip and a 128-wide tile runs part empty; the channel-parallel kernel (lanes
    // split K per pixel) has the parallelism there.  S2V_HALO_MIN_BLOCKS overrides (tuning).
    const long long blocks = (long long)p->n * cdiv(p->ow, 128) * cdiv(p->oh, 8);
    if (blocks < tune_get(S2V_TUNE_HALO_MIN_BLOCKS)) return 0;
    return p->kh;
}

// channel splits of the halo kernel: about three blocks per CU, at least 8 channels per split
static int halo_splits(const s2v_conv_params *p, int &per) {
    const long long blocks = (long long)p->n * cdiv(p->ow, 128) * cdiv(p->oh, 8);
    const int cus = plan_cus();
    const int quads = p->cin / 4;
    int s = blocks >= 3LL * cus ? 1 : (int)((3LL * cus + blocks - 1) / blocks);
    if (s > quads / 2) s = quads / 2;
    if (s < 1) s = 1;
    per = 4 * ((quads + s - 1) / s);
    return (p->cin + per - 1) / per;
}

// Split-precision heads (conv_head.hip): plain 5x5 / 7x7 heads over 32 or 64k <= 512 channels
static bool head_x3_ok(const s2v_conv_params *p) {
    if (!head_x3_on() || p->prec == S2V_PREC_F32 || p->x_split || p->force_tile || !p->wt_x3 || ((uintptr_t)p->wt_x3 % 16))
        return false;
    return plain_head(p) && (p->kh == 7 || p->kh == 5) && (p->cin == 32 || p->cin % 64 == 0) && p->cin <= 512 &&
           !p->out_pool && !p->d2s_cout;
}
// output rows per conv_head_x3 block: 16, halved while the grid is under two blocks per CU (>= 4).
// (device_cus(), not plan_cus(): without a device this never halves.  The one place the planner reads
// the raw count; kept, since changing it would change a launch parameter.)
static int head_rows(const s2v_conv_params *p) {
    const long long strips = cdiv(p->ow, 32 - p->kw + 1);
    int th = 16;
    const long long groups = p->cin > 64 ? p->cin / 64 : 1;
    while (th > 4 && (long long)p->n * strips * groups * cdiv(p->oh, th) < 2LL * device_cus()) th /= 2;
    return th;
}

// LDS weights of conv_small_cpar when the filter is small next to the block's input (<= 16 KB: ToRGB
// 1x1s); the 7x7 heads keep global (L1-resident) weight reads.  Per-batch-entry weights need every
// block inside one entry (M % pixels-per-block == 0).
static bool cpar_lw(int co, int K, long long w_bs, int batch, int M, int tpp) {
    return (size_t)co * K * sizeof(float) <= 16 * 1024 && (w_bs == 0 || batch == 1 || M % (256 / tpp) == 0);
}

// lanes per output pixel of conv_small_cpar: 8 lanes per pixel (each lane walks cin/32 float4s): 3
// shuffle levels per output instead of 5-6 with one float4 per lane, 128-byte contiguous row pieces
// per load instruction.  Below 128 channels fewer lanes share a pixel so every lane still has >= 4
// float4s in flight per tap: with one float4 per lane (32-channel ToRGB heads at 2048^2, RealESRNet's
// conv_last) the kernel was latency-bound at 1.5 TB/s.
static int cpar_lanes(int cin) { return cin >= 128 ? 8 : cin >= 64 ? 4 : cin >= 32 ? 2 : 4; }

// 4-channel 1x1 / 3x3 convs on the exact-fp32 MFMA kernel (conv_k4.hip) in every precision mode: stride 1,
// zero "same" padding or none (the kernel bounds-checks every tap against the input, so the unpadded conv is the
// padded one's interior), 32k <= 256 output channels, a plain epilogue (scale, shift, per-pixel add, activation)
static bool k4_ok(const s2v_conv_params *p) {
    if (!k4_on() || p->cin != 4 || p->kh != p->kw || (p->kh != 1 && p->kh != 3) || p->force_tile || p->b_kn || p->x_split)
        return false;
    if (p->in_mode != S2V_IN_DIRECT || p->pad_mode != S2V_PAD_ZERO || p->sh != 1 || p->sw != 1 || p->dh != 1 ||
        p->dw != 1 || !((p->ph == p->kh / 2 && p->pw == p->kw / 2) || (p->ph == 0 && p->pw == 0)))
        return false;
    if (p->cout % 32 || p->cout > 256 || p->in_scale || p->pre_act != S2V_ACT_NONE || p->nc_scale || p->res ||
        p->post_mul || p->dup_src || p->out_pool || p->out_step > 1 || p->d2s_cout > 0)
        return false;
    if (!p->wt || p->kpad < p->kh * p->kw * 4 || p->xcs % 4 || ((uintptr_t)p->x % 16) || p->x_bs % 4) return false;
    return (long long)p->n * p->oh * p->ow < (1LL << 31);
}

// conv_smallk geometry: threads per pixel (cout / 4 channel quads, at most 64) and quads per thread
static bool smallk_cfg(const s2v_conv_params *p, int M, int K, int &tppx, int &qpt) {
    if (p->b_kn || p->force_tile || p->out_pool || p->cout < 8 || (p->cout & 3) || K > 64 || !vec4_input(p)) return false;
    // multi-tap filters on 4k-channel inputs go to the split-precision implicit GEMM even at K <= 64
    // (measured on MI355X, r02: 3x3 4 -> 256 at 200^2 776 -> 336 us, 4 -> 64 at 512^2 602 -> 361 us,
    // at 96^2 74 -> 32 us; the 1x1 4 -> 256 layer stays here, 415 us against 491 us)
    if (p->prec != S2V_PREC_F32 && p->kh * p->kw > 1) return false;
    // 1x1 convs on >= 32 channels too (ResNet-50 layer1 64 -> 64 / 64 -> 256 at 56^2: VALU-bound here)
    if (p->prec != S2V_PREC_F32 && K >= 32) return false;
    const int quads = p->cout / 4;
    if (quads & (quads - 1)) return false;                       // power of two
    // one output quad per thread, up to 64 threads per pixel (measured on MI355X: 64 lanes x 1 quad
    // beat 4 lanes x 16 quads and 4-pixel register blocking on the 256-channel image layers, r02)
    tppx = quads < 64 ? quads : 64;
    qpt = quads / tppx;
    if (qpt > 2 || (size_t)K * p->cout * sizeof(float) > 64 * 1024) return false;
    return p->w_bs == 0 || batch_of(p) == 1 || M % (256 / tppx) == 0;
}

// pixels per block = iters x (256 / tppx): up to 16 iterations, and a divisor of M when each
// batch entry has its own weights (a block never straddles two entries)
static int smallk_iters(const s2v_conv_params *p, int M, int tppx) {
    const bool per_entry = p->w_bs != 0 && batch_of(p) > 1;
    int it = 16;
    while (it > 1 && per_entry && M % (it * (256 / tppx)) != 0) it /= 2;
    return it;
}

static bool is_smallk(const s2v_conv_params *p) {
    const long long m = (long long)p->n * p->oh * p->ow, k = (long long)p->kh * p->kw * p->cin;
    int tppx, qpt;
    return m < (1LL << 31) && k <= 64 && smallk_cfg(p, (int)m, (int)k, tppx, qpt);
}
static bool tiled_x3(const s2v_conv_params *p) {
    return p->prec != S2V_PREC_F32 && !(use_direct(p) && !p->force_tile) && !is_smallk(p) && !k4_ok(p);
}

// 0: fast direct path, 1: generic float4 gather, 2: scalar gather, 3: reflect / nearest-x2 rows
static int a_mode(const s2v_conv_params *p) {
    const bool vec = (p->cin % 4 == 0) && (p->xcs % 4 == 0) && (((uintptr_t)p->x % 16) == 0) && (p->x_bs % 4 == 0);
    if (!vec) return 2;
    const bool simple_pre = (p->pre_act == S2V_ACT_NONE || p->pre_act == S2V_ACT_RELU || p->pre_act == S2V_ACT_LRELU) &&
                            (!p->in_scale || (p->in_scale_ns % 4 == 0 && ((uintptr_t)p->in_scale % 16) == 0));
    if (p->cin % 32 == 0 && p->in_mode != S2V_IN_TRANSPOSED && simple_pre && !p->b_kn)
        return (p->pad_mode == S2V_PAD_ZERO && p->in_mode == S2V_IN_DIRECT) ? 0 : 3;
    if (p->cin % 32 == 0 && p->in_mode == S2V_IN_DIRECT && p->pad_mode == S2V_PAD_ZERO && simple_pre) return 0;
    return 1;
}

// buffer-load extents of one batch slab of x / of the packed weights
static long long x_extent_bytes(const s2v_conv_params *p) {
    return ((long long)p->n * p->h * p->w - 1) * p->xcs * 4 + (long long)p->cin * 4;
}
static long long w_extent_bytes(const s2v_conv_params *p) { return (long long)p->npad * p->kpad * 4; }

// 1x1 convs over cin % 8 == 0 (not % 32) channels take the buffer-load path too: the last 32-channel
// K-slice is partial and the lanes whose 8 channels lie past cin load zeros (r04: LNet's 48^2 st2 over
// 48 channels ran the per-row float4 gather)
static bool x3_partial_1x1(const s2v_conv_params *p) {
    return p->kh == 1 && p->kw == 1 && p->cin % 8 == 0 && p->cin % 32 != 0 && p->in_mode == S2V_IN_DIRECT &&
           p->pad_mode == S2V_PAD_ZERO && !p->b_kn && !p->x_split && a_mode(p) == 1 && p->pre_act == S2V_ACT_NONE &&
           !p->in_scale;   // (an input scale would be read past cin by the masked lanes' prologue)
}

// The split-precision kernels' A-operand mode: AMODE 0 becomes 4 (buffer loads, conv_x3_impl.hpp)
// when the tile stages A wide (BM a multiple of 16 * waves), the filter has <= 32 taps and the x
// slab / packed weights fit the 2^31-byte offsets.
static int x3_amode(const s2v_conv_params *p, const TileCfg &t) {
    const int am = x3_partial_1x1(p) ? 0 : a_mode(p);
    if (am != 0 || p->b_kn || p->kh * p->kw > 32 || t.bm % (16 * t.nw) != 0) return a_mode(p);
    // past the 2^31-byte buffer offsets: the gather path the conv would take without buffer loads (a_mode,
    // never AMODE 0 for a partial 1x1, which assumes whole 32-channel K-slices)
    if (x_extent_bytes(p) >= (1LL << 31) || w_extent_bytes(p) >= (1LL << 31)) return a_mode(p);
    return 4;
}

// What conv_x3_nar and conv_x3_halo share: the AMODE 4 addressing (direct zero-padded conv, whole 32-channel
// slices, 2^31-byte offsets), packed weights covering every 64-row B slab, no pooled epilogue
static bool direct_a_ok(const s2v_conv_params *p) {
    return tiled_x3(p) && !p->b_kn && !p->x_split && a_mode(p) == 0 && p->cin % 32 == 0 && !p->out_pool &&
           x_extent_bytes(p) < (1LL << 31) && w_extent_bytes(p) < (1LL << 31) && (long long)cdiv(p->cout, 64) * 64 <= p->npad;
}
// conv_x3_nar: <= 32 taps, and with an input modulation every 256-row tile inside one image (its s[n, c]
// loads are per tile)
static bool nar_ok(const s2v_conv_params *p) {
    return direct_a_ok(p) && p->kh * p->kw <= 32 && (!p->in_scale || (p->oh * p->ow) % 256 == 0);
}
// conv_x3_halo: 3x3 stride 1 pad 1 (a halo patch never straddles two images: no in_scale condition)
static bool halo_ok(const s2v_conv_params *p) {
    return direct_a_ok(p) && p->kh == 3 && p->kw == 3 && p->sh == 1 && p->sw == 1 && p->dh == 1 && p->dw == 1 &&
           p->ph == 1 && p->pw == 1;
}

// output pixels / patch-grid pixels of conv_x3_halo's TH x 64 patches (ragged images run part-empty patches)
static double halo_fill(const s2v_conv_params *p, int th) {
    return (double)p->oh * p->ow / ((double)cdiv(p->oh, th) * th * cdiv(p->ow, 64) * 64);
}

static bool x3_kind_ok(const s2v_conv_params *p, int kind) {
    if (kind == 4) return halo_ok(p) && p->oh % 8 == 0;
    if (kind == 5) return halo_ok(p) && (long long)cdiv(p->cout, 128) * 128 <= p->npad;
    return kind == 0 || (kind == 3 ? halo_ok(p) : nar_ok(p));
}

// Persistent blocks of a launch under s2v_conv_params.grid_cap: the 256x256 buffer-load split-precision
// tile only (conv_x3_impl.hpp x3_has_persist), when the tile grid exceeds the cap; 0 = one block per tile
static int persist_blocks(const s2v_conv_params *p, const Plan &pl) {
    // (not with the SFT / second-output extras: the persistent kernel is built without them)
    if (p->grid_cap <= 0 || p->b_kn || pl.tile != 0 || pl.amode != 4 || p->post_mul || p->dup_src) return 0;
    const long long cap = p->grid_cap & ~7LL;
    return cap > 0 && tile_blocks(pl, pl.t) * pl.splits > cap ? (int)cap : 0;
}

// ------------------------------------------------------------------ plans
// split-K factor of a chosen tile: force_splits, or enough splits for two blocks per CU when the grid has fewer
// than ``below`` blocks, with at least 8 K-slices per split (finish_plan clamps to >= 1)
static int fill_splits(const s2v_conv_params *p, const Plan &pl, long long blocks, long long below) {
    if (p->force_splits > 0) return p->force_splits;
    const int s = blocks < below ? (int)((2LL * plan_cus() + blocks - 1) / blocks) : 1;
    return s > pl.ktiles / 8 ? pl.ktiles / 8 : s;
}

static void finish_plan(Plan &pl, int splits) {
    if (pl.kslab > 1) {                  // splits over whole groups of kslab K-slices (conv_x3_halo: 9 taps)
        const int groups = pl.ktiles / pl.kslab;
        if (splits > groups) splits = groups;
        if (splits < 1) splits = 1;
        pl.tps = (groups + splits - 1) / splits * pl.kslab;
        pl.splits = (pl.ktiles + pl.tps - 1) / pl.tps;
        return;
    }
    if (splits > pl.ktiles) splits = pl.ktiles;
    if (splits < 1) splits = 1;
    pl.tps = (pl.ktiles + splits - 1) / splits;
    pl.splits = (pl.ktiles + pl.tps - 1) / pl.tps;
}

// A split-precision tile plan: the kernel family and instance parameters of kX3Tiles[tile]
static void finish_x3(const s2v_conv_params *p, Plan &pl, int tile, int splits) {
    const X3Cfg &c = kX3Tiles[tile];
    pl.tile = tile;
    pl.t = c.t;
    pl.route = c.kind >= 3 ? Route::X3Halo : c.kind >= 1 ? Route::X3Nar : Route::X3Tile;
    if (c.kind >= 3) {
        pl.kslab = 9;
        pl.th = c.kind == 4 ? 8 : 4;
        pl.wn = c.kind == 5 ? 2 : 1;
    }
    finish_plan(pl, splits);
    pl.amode = c.kind >= 3 ? 8 : c.kind >= 1 ? 5 + c.kind : x3_amode(p, c.t);
    if (c.kind >= 1 || pl.amode == 4) {
        pl.x_bytes = (unsigned)x_extent_bytes(p);
        pl.w_bytes = (unsigned)w_extent_bytes(p);
    }
    if (pl.route == Route::X3Tile) pl.persist = persist_blocks(p, pl);
}

// Split-bf16 planner: minimise a simple time model over (tile, split-K):
//   T = ceil(blocks / (CUs * bpc)) * t_block + splitk_reduce
// with t_block = one block's share of the tile's sustained full-chip rate (kX3Tiles).
static void make_plan_x3(const s2v_conv_params *p, Plan &pl) {
    const int M = pl.M, batch = pl.batch;
    const int cus = plan_cus();
    if (p->force_tile > 0) {
        const int tile = p->force_tile - 1;
        return finish_x3(p, pl, tile, fill_splits(p, pl, tile_blocks(pl, kX3Tiles[tile].t), 2LL * cus));
    }
    // 3x3 stride-1 layers of <= 128 output channels over 64-wide rows (the enhancers' and DNet's 128^2 -
    // 512^2 layers): the halo-staged spatial patch kernel, measured 20-30 % faster than every implicit-GEMM
    // tile on them (4x512^2 64 -> 64: 356 vs 444 us, 128 -> 64: 547 vs 697, 4x256^2 128 -> 128: 292 vs 381,
    // profiles/r05_halo_sweep.txt), whenever the grid fills the chip without split-K
    // (<= 32 output channels stay on the 32-column tiles: half of a 64-column halo block would be idle,
    // 4x512^2 64 -> 32: 320 us against 277 us on 128x32)
    if (halo_ok(p) && p->cout > 32 && p->cout <= 128 && halo_fill(p, 4) >= 0.85) {
        const long long blocks = (long long)p->n * cdiv(p->oh, 4) * cdiv(p->ow, 64) * cdiv(p->cout, 64) * batch;
        // 65..128 output channels: one block per 128 columns (two 64-channel wave columns share the halo):
        // 4x256^2 128 -> 128 279 vs 291 us (profiles/r05_halo_sweep.txt); <= 64: the 4-wave 64-column block
        const int kind = p->cout > 64 && x3_kind_ok(p, 5) ? 5 : 3;
        // ... but large 65..128-channel layers stay on 512x128: 16x400^2 128 -> 128 2189 us there against
        // 2595 / 2418 us on the halo blocks (profiles/r05_halo_sweep.txt)
        const bool big_n128 = p->cout > 64 && (long long)p->n * p->oh * p->ow * batch >= (1LL << 20);
        if (blocks >= 2LL * cus && !big_n128) {
            for (int i = 0; i < kNumX3; ++i)
                if (kX3Tiles[i].kind == kind) return finish_x3(p, pl, i, 1);
        }
    }
    if (pl.ktiles <= 4 && !p->b_kn && tune_get(S2V_TUNE_SMALLK_TILE)) {
        // K <= 128 (image-input layers): the launch is output-write / gather bound, the throughput
        // model does not apply.  One N tile covering cout reads A once; measured on MI355X (r02):
        // 4 -> 256 3x3 at 200^2 256x256 336 us (128x128 497), 4 -> 64 at 96^2 64x64 32 us (128x64 43)
        // (small M — LNet's 12^2 1x1 convs — keeps the throughput model: it needs the blocks)
        int t = p->cout > 128 ? 0 : (p->cout > 64 ? 1 : 4);
        const TileCfg &c = kX3Tiles[t].t;
        if ((long long)cdiv(p->cout, c.bn) * c.bn <= p->npad && tile_blocks(pl, c) >= 4LL * cus) return finish_x3(p, pl, t, 1);
    }
    double best = 1e30;
    int bt = 8, bs = 1;                                      // 512x128: the planner's fallback
    const int am = a_mode(p);
    for (int i = 0; i < kNumX3; ++i) {
        const X3Cfg &c = kX3Tiles[i];
        if (c.tflops <= 0.f) continue;                          // forced-only configurations
        if (!x3_kind_ok(p, c.kind)) continue;
        if (p->b_kn && c.t.nw != 4) continue;
        if (c.t.bm >= 256 && c.t.bn >= 128 && am != 0 && am != 3) continue;   // generic gathers spill there
        // the 256 / 512-row narrow-N tiles on per-row gathers: measured slower than 128x64 (256x64, r02)
        if (c.t.bm >= 256 && c.t.bn <= 64 && am != 0) continue;
        if (!p->b_kn && (long long)cdiv(p->cout, c.t.bn) * c.t.bn > p->npad) continue;   // weight rows
        const long long tiles = tile_blocks(pl, c.t);
        const double slots = (double)cus * c.bpc;
        for (int s = 1; s <= 16; s *= 2) {
            if (s > 1 && (p->force_splits > 0 || s > pl.ktiles / 4)) break;
            if (p->force_splits > 0) s = p->force_splits;
            const int tps = (pl.ktiles + s - 1) / s;
            const long long r512 = (c.t.bm == 512) ? tune_get(S2V_TUNE_X3_RATE_512) : 0;
            const double rate = r512 > 0 ? (double)r512 : c.tflops;
            const double t_block = 2.0 * c.t.bm * c.t.bn * 32.0 * tps / (rate * 1e12 / slots);
            double t = std::ceil((double)(tiles * s) / slots) * t_block;
            if (s > 1) t += 4e-6 + (double)batch * M * p->cout * 4.0 * (s + 1) / 4e12;
            if (t < best * 0.97) {   // prefer the earlier (larger) tile / fewer splits on near ties
                best = t;
                bt = i;
                bs = s;
            }
            if (p->force_splits > 0) break;
        }
    }
    finish_x3(p, pl, bt, bs);
}

static int glds_cfg(const s2v_conv_params *p) {
    const int forced = (int)tune_get(S2V_TUNE_GLDS_TILE);   // tuning override (tools/glds_sweep.sh)
    if (forced >= 0 && forced < (int)(sizeof(kGlds) / sizeof(kGlds[0]))) {
        const GldsCfg &c = kGlds[forced];
        if ((long long)cdiv(p->cout, c.bn) * c.bn <= p->npad) return forced;
    }
    if (p->cout > 128 && (long long)cdiv(p->cout, 256) * 256 <= p->npad) return 0;
    // N <= 128: 512x128 (128x64 per wave) over 256x128 (64x64 per wave, 33 % more LDS reads per
    // MFMA): 400^2 256 -> 128 4330 vs 4648 us, 128 -> 128 2543 vs 2749 us (r02)
    const long long m = (long long)p->n * p->oh * p->ow * batch_of(p);
    return m >= 512LL * 1024 ? 2 : 1;
}

static void make_plan_glds(const s2v_conv_params *p, Plan &pl) {
    pl.route = Route::Glds;
    pl.tile = glds_cfg(p);
    const GldsCfg &c = kGlds[pl.tile];
    pl.t = TileCfg{c.bm, c.bn, c.wm, 8, c.nst, 0};
    pl.amode = 5;
    finish_plan(pl, fill_splits(p, pl, tile_blocks(pl, pl.t), plan_cus()));
}

static void make_plan_igemm(const s2v_conv_params *p, Plan &pl) {
    const long long target = 2LL * plan_cus();
    int cands[kNumTiles];
    int nc = 0;
    if (p->force_tile > 0) {
        cands[nc++] = p->force_tile - 1;
    } else if (p->cout <= 32) {
        cands[nc++] = 5;
    } else if (p->cout <= 64) {
        cands[nc++] = 1; cands[nc++] = 3;
    } else {
        cands[nc++] = 0; cands[nc++] = 1; cands[nc++] = 2; cands[nc++] = 3;
    }
    pl.tile = cands[nc - 1];               // the first candidate that fills the chip, else the smallest
    for (int i = 0; i < nc; ++i)
        if (tile_blocks(pl, kTiles[cands[i]]) >= target) {
            pl.tile = cands[i];
            break;
        }
    pl.route = Route::Igemm;
    pl.t = kTiles[pl.tile];
    pl.amode = a_mode(p);
    finish_plan(pl, fill_splits(p, pl, tile_blocks(pl, pl.t), target));
}

// An unsplit plan of the launch's GEMM with no route yet
static Plan new_plan(const s2v_conv_params *p, int M, int K) {
    Plan pl{};
    pl.M = M; pl.K = K; pl.batch = batch_of(p);
    pl.cout = p->cout; pl.prec = p->prec; pl.bkn = p->b_kn != 0;
    pl.kslab = 1; pl.ktiles = (K + 31) / 32; pl.splits = 1; pl.tps = pl.ktiles;
    return pl;
}

// The one place that decides the route and every instance parameter of a validated launch.
static Plan make_plan(const s2v_conv_params *p_in, int M, int K) {
    s2v_conv_params q = *p_in;
    // single-pass f16 plans exactly as f16x3 (same route, tile, splits, persistence: the predicates below see
    // S2V_PREC_F16X3); the plan's prec then says what the launch really runs
    if (q.prec == S2V_PREC_F16) q.prec = S2V_PREC_F16X3;
    if (q.out_pool) q.force_splits = 1;          // the pooled epilogue needs whole-K tiles
    const s2v_conv_params *p = &q;
    Plan pl = new_plan(p, M, K);
    int tppx, qpt;
    if (p->x_split) {
        make_plan_glds(p, pl);
    } else if (head_x3_ok(p)) {
        pl.route = Route::HeadX3;
        pl.splits = p->cin > 64 ? p->cin / 64 : 1;     // 64-channel groups, folded by splitk_reduce
        pl.fsize = p->kh;
        pl.ncs = p->cin == 32 ? 1 : 2;
        pl.rows = head_rows(p);
    } else if (use_direct(p) && !p->force_tile) {
        if ((pl.fsize = halo_ks(p)) != 0) {
            pl.route = Route::HaloSmall;
            pl.splits = halo_splits(p, pl.tps);        // tps: channels per split
        } else if (vec4_input(p)) {
            pl.route = Route::SmallCpar;
            pl.lanes = cpar_lanes(p->cin);
            pl.lds_w = cpar_lw(p->cout, K, p->w_bs, pl.batch, M, pl.lanes);
        } else {
            pl.route = Route::DirectSmall;
        }
    } else if (k4_ok(p)) {                             // conv_k4_mfma (fp32 MFMA, no split-K)
        pl.route = Route::K4;
        pl.kt = p->kh * p->kw;
    } else if (smallk_cfg(p, M, K, tppx, qpt)) {
        // conv_smallk4<QPT, KT> for 4-channel 1x1 / 3x3 inputs
        pl.kt = p->cin == 4 && p->kh == p->kw && (p->kh == 1 || p->kh == 3) ? p->kh * p->kw : 0;
        pl.route = pl.kt ? Route::SmallK4 : Route::SmallK;
        pl.tppx = tppx;
        pl.qpt = qpt;
        pl.iters = smallk_iters(p, M, tppx);
    } else if (tiled_x3(p)) {
        make_plan_x3(p, pl);
    } else {
        make_plan_igemm(p, pl);
    }
    if (pl.splits > 1) pl.ws_bytes = (size_t)pl.batch * pl.splits * (size_t)M * p->cout * sizeof(float);
    // the families with single-pass (ELT 2) instances: conv_igemm_x3 (plain / persistent) and conv_x3_halo; every
    // other split-precision family (conv_x3_nar, conv_head_x3, conv_glds_x3) runs the mode as f16x3
    if (p_in->prec == S2V_PREC_F16 && (pl.route == Route::X3Tile || pl.route == Route::X3Halo)) pl.prec = S2V_PREC_F16;
    return pl;
}

static bool pow2_or_zero(float v) {
    int e;
    return v == 0.f || (v > 0.f && std::frexp(v, &e) == 0.5f);
}

static int validate(const s2v_conv_params *p, int &M, int &K) {
    S2V_REQUIRE(p && p->x && p->y, "conv2d: null pointer");
    S2V_REQUIRE(pow2_or_zero(p->x_scale), "conv2d: x_scale must be 0 or a positive power of two, got %g", p->x_scale);
    S2V_REQUIRE(!p->x_split || p->x_scale == 0.f || p->x_scale == 1.f,
                "conv2d: split-layout inputs carry no x_scale (split them already scaled)");
    S2V_REQUIRE(!p->stamps || (p->stamp_ctr && p->stamp_reps > 0 && p->stamp_slot >= 0 &&
                               p->stamp_slot < p->stamp_stride),
                "conv2d: launch stamps need stamp_ctr, stamp_reps > 0 and 0 <= stamp_slot < stamp_stride");
    S2V_REQUIRE(p->prec == S2V_PREC_F32 || p->prec == S2V_PREC_BF16X3 || p->prec == S2V_PREC_F16X3 ||
                    p->prec == S2V_PREC_F16,
                "conv2d: bad prec %d", p->prec);
    S2V_REQUIRE(pow2_or_zero(p->wt_scale), "conv2d: wt_scale must be 0 or a positive power of two, got %g", p->wt_scale);
    const bool x3 = tiled_x3(p);
    S2V_REQUIRE(p->force_tile >= 0 && p->force_tile <= (x3 ? kNumX3 : kNumTiles),
                "conv2d: bad force_tile %d", p->force_tile);
    S2V_REQUIRE(!(x3 && p->b_kn && p->force_tile > 0 && kX3Tiles[p->force_tile - 1].t.nw != 4),
                "conv2d: b_kn operands need a 4-wave split-bf16 tile (force_tile 4..6)");
    S2V_REQUIRE(!(x3 && p->force_tile > 0 && !x3_kind_ok(p, kX3Tiles[p->force_tile - 1].kind)),
                "conv2d: force_tile %d (conv_x3_nar / conv_x3_halo) needs a direct zero-padded conv, cin %% 32 == 0, "
                "<= 32 taps, no pooling, packed weights over whole 64-row slabs, 2^31-byte offsets and, with "
                "in_scale, oh * ow %% 256 == 0; conv_x3_halo also 3x3 stride 1 pad 1 (ragged images run partly empty "
                "patches), and its 8-row form oh %% 8 == 0",
                p->force_tile);
    if (x3 && p->force_tile > 0) {
        // a forced tile must not read weight rows past the packed [npad] rows (the planner never
        // picks such a tile: the kernels load whole BN-row slabs of B without a row guard)
        const TileCfg &t = kX3Tiles[p->force_tile - 1].t;
        S2V_REQUIRE(!p->b_kn ? (long long)cdiv(p->cout, t.bn) * t.bn <= p->npad : true,
                    "conv2d: force_tile %d (BN %d) needs npad >= %d, got %d", p->force_tile, t.bn,
                    cdiv(p->cout, t.bn) * t.bn, p->npad);
    }
    if (p->x_split) {
        S2V_REQUIRE(p->prec == S2V_PREC_BF16X3 || p->prec == S2V_PREC_F16X3 || p->prec == S2V_PREC_F16,
                    "conv2d: x_split needs prec BF16X3 / F16X3");
        S2V_REQUIRE(!p->b_kn && p->in_mode == S2V_IN_DIRECT && p->pad_mode == S2V_PAD_ZERO && p->cin % 32 == 0 &&
                        p->kh * p->kw <= 32 && !p->in_scale && p->pre_act == S2V_ACT_NONE && p->xcs % 4 == 0 &&
                        ((uintptr_t)p->x % 16) == 0 && p->x_bs % 4 == 0 && p->force_tile == 0,
                    "conv2d: x_split needs a direct zero-padded conv, cin %% 32 == 0, <= 32 taps, packed weights, "
                    "no in_scale / pre_act / force_tile, xcs %% 4 == 0 and a 16-byte aligned x");
        S2V_REQUIRE(p->wt_x3 && ((uintptr_t)p->wt_x3 % 16) == 0, "conv2d: x_split needs 16B-aligned wt_x3");
    } else if (x3 && !p->b_kn)   // the kernels read the pre-split packed weights; b_kn matrices are split on the fly
        S2V_REQUIRE(p->wt_x3 && ((uintptr_t)p->wt_x3 % 16) == 0, "conv2d: split precisions need 16B-aligned wt_x3");
    else
        S2V_REQUIRE(p->wt != nullptr, "conv2d: null weights");
    S2V_REQUIRE(p->n > 0 && p->h > 0 && p->w > 0 && p->cin > 0 && p->cout > 0 && p->oh > 0 && p->ow > 0,
                "conv2d: bad shape n=%d h=%d w=%d cin=%d cout=%d oh=%d ow=%d", p->n, p->h, p->w, p->cin,
                p->cout, p->oh, p->ow);
    S2V_REQUIRE(p->kh > 0 && p->kw > 0 && p->sh > 0 && p->sw > 0 && p->dh > 0 && p->dw > 0, "conv2d: bad kernel");
    S2V_REQUIRE(p->xcs >= p->cin && p->ycs >= (p->d2s_cout > 0 ? p->d2s_cout : p->cout),
                "conv2d: channel stride smaller than channels");
    S2V_REQUIRE(p->in_mode >= 0 && p->in_mode <= 2, "conv2d: bad in_mode %d", p->in_mode);
    S2V_REQUIRE(!(p->pad_mode == S2V_PAD_REFLECT && p->in_mode == S2V_IN_TRANSPOSED),
                "conv2d: reflect padding only with direct or nearest-x2 input");
    {
        const int up = p->in_mode == S2V_IN_NEAREST_UP2 ? 2 : 1;   // reflection happens in the upsampled frame
        S2V_REQUIRE(!(p->pad_mode == S2V_PAD_REFLECT && (p->ph >= up * p->h || p->pw >= up * p->w)),
                    "conv2d: reflect pad must be smaller than the input");
    }
    const long long m = (long long)p->n * p->oh * p->ow;
    const long long k = (long long)p->kh * p->kw * p->cin;
    S2V_REQUIRE(m < (1LL << 31) && k < (1LL << 31), "conv2d: problem too large");
    M = (int)m;
    K = (int)k;
    if (p->b_kn) {
        S2V_REQUIRE(p->ldb >= p->cout, "conv2d: ldb < cout");
        S2V_REQUIRE(p->ldb % 4 == 0 && ((uintptr_t)p->wt % 16) == 0, "conv2d: b_kn needs ldb%%4==0, 16B aligned");
    } else {
        S2V_REQUIRE(p->kpad >= k && p->kpad % 32 == 0, "conv2d: kpad=%d must be >= K=%lld and %%32", p->kpad, k);
        S2V_REQUIRE(p->npad >= p->cout && p->npad % 128 == 0, "conv2d: npad=%d must be >= cout and %%128", p->npad);
        S2V_REQUIRE(x3 || ((uintptr_t)p->wt % 16) == 0, "conv2d: weights must be 16B aligned");
    }
    if (p->res) S2V_REQUIRE(p->res_cs >= p->cout, "conv2d: res_cs < cout");
    if (p->out_pool) {
        S2V_REQUIRE(p->oh % 2 == 0 && p->ow % 2 == 0, "conv2d: out_pool needs even output sizes");
        S2V_REQUIRE(!p->res && !p->nc_scale && !p->pix_add && p->out_step <= 1 && p->force_splits <= 1,
                    "conv2d: out_pool takes no res / nc_scale / pix_add / strided output / K split");
        S2V_REQUIRE(p->x_split || (!(use_direct(p) && !p->force_tile) && !is_smallk(p)),
                    "conv2d: out_pool needs the implicit-GEMM path");
    }
    if (p->post_mul || p->dup_src) {
        S2V_REQUIRE(p->out_step <= 1 && !p->out_pool && p->d2s_cout <= 0 && p->batch <= 1 && p->cout > 4,
                    "conv2d: post_mul / dup_src need a dense output (no strided / pooled / depth-to-space / batched) "
                    "and cout > 4");
        S2V_REQUIRE(!p->post_mul || (p->post_add && p->post_c0 >= 0 && p->post_c0 < p->cout &&
                                     p->post_cs >= p->cout - p->post_c0),
                    "conv2d: post_mul needs post_add, 0 <= post_c0 < cout and post_cs >= cout - post_c0");
        S2V_REQUIRE(!p->dup_src || (p->dup_cs >= p->cout && p->dup_off >= p->cout && p->dup_off + p->cout <= p->ycs),
                    "conv2d: dup_src needs dup_cs >= cout and cout <= dup_off <= ycs - cout");
    }
    if (p->d2s_cout > 0)
        S2V_REQUIRE(p->out_step == 2 && p->cout == 4 * p->d2s_cout && !p->res && !p->out_pool && !p->nc_scale,
                    "conv2d: depth-to-space output needs out_step 2, cout == 4 * d2s_cout, no res / pool / nc_scale");
    if (p->out_step > 1) {
        S2V_REQUIRE(!p->pix_add || p->d2s_cout > 0, "conv2d: strided output cannot take pix_add");
        S2V_REQUIRE(!p->res || (p->res == p->y && p->res_cs == p->ycs && p->res_oy == 0 && p->res_ox == 0),
                    "conv2d: strided output only takes an in-place residual (res == y)");
        S2V_REQUIRE(p->cout > 4 || p->x_split, "conv2d: strided output needs the implicit-GEMM path (cout > 4)");
        S2V_REQUIRE(p->out_full_h >= (p->oh - 1) * p->out_step + 1 && p->out_full_w >= (p->ow - 1) * p->out_step + 1,
                    "conv2d: strided output exceeds out_full_h/w");
    }
    return 0;
}

int plan_conv(const s2v_conv_params *p, Plan &pl) {
    int M, K;
    const int rc = validate(p, M, K);
    if (rc) return rc;
    pl = make_plan(p, M, K);
    return 0;
}

// The eleven ints of s2v_conv2d_plan (include/s2v.h)
void encode_plan(const Plan &pl, int *out) {
    for (int i = 0; i < 11; ++i) out[i] = 0;
    out[1] = pl.cout;
    out[5] = pl.splits;
    switch (pl.route) {
        case Route::K4: out[4] = 4000 + pl.kt; return;               // conv_k4_mfma<KT>
        case Route::SmallK:                                          // conv_smallk<QPT, 1>
        case Route::SmallK4:                                         // conv_smallk4<QPT, KT>
            out[2] = -pl.qpt; out[3] = 1; out[4] = pl.kt ? 2000 + pl.kt : 0;
            return;
        case Route::HeadX3:                                          // conv_head_x3<prec - 1, CO, KS, NCS>
            out[2] = pl.ncs; out[4] = 3000 + pl.fsize;
            out[6] = pl.prec;
            return;
        case Route::HaloSmall: out[4] = 1000 + pl.fsize; return;    // conv_halo_small<CO, KS>
        case Route::SmallCpar: out[2] = pl.lanes; out[3] = pl.lds_w; return;   // conv_small_cpar<CO, TPP, LW>
        case Route::DirectSmall: return;                             // conv_direct_small<CO>
        default: break;
    }
    out[0] = pl.t.bm; out[1] = pl.t.bn; out[2] = pl.t.wm;
    out[3] = pl.amode;
    out[4] = pl.bkn;
    out[6] = pl.route == Route::Igemm ? 0 : pl.prec;
    out[7] = pl.t.nw; out[8] = pl.t.ks; out[9] = pl.t.pf;
    out[10] = pl.persist;
}

// ------------------------------------------------------------------ grouped launches
// A group of independent split-precision convs (s2v_conv2d_group: LNet's FFC conv_to_l, l2g and the
// spectral branch's first 1x1, which all read the block input) as one launch on one tile
// configuration, each member with its own split-K factor, plus one launch folding every member's
// partials.  Plan: minimise  rounds * (T0 + max_p tps_p * t_slice) + [reduce]  over the grouped tiles
// and per-member splits in {1, 2, 4, 8, 16}, where t_slice = max(the tile's per-slice latency floor,
// its share of the full-chip rate) — the latency floor is what one block alone on a CU takes per
// 32-deep K slice (measured on MI355X r04, graph-timed: 0.5 us for the 4-wave tiles).
static bool group_member_ok(const s2v_conv_params *p, int cfg) {
    return tiled_x3(p) && !p->b_kn && !p->x_split && p->grid_cap == 0 && p->force_tile == 0 && !p->out_pool &&
           (p->batch <= 1) && x3_amode(p, kX3Tiles[cfg].t) == 4 && !p->in_scale && p->pre_act == S2V_ACT_NONE &&
           !p->post_mul && !p->dup_src;       // the grouped kernel is built without the epilogue extras
}

int plan_group(const s2v_conv_params *ps, int n, GroupPlan &gp) {
    S2V_REQUIRE(ps && n >= 1 && n <= kPlanGroupMax, "conv2d_group: 1..%d members", kPlanGroupMax);
    int M[kPlanGroupMax], K[kPlanGroupMax], splits[kPlanGroupMax];
    for (int i = 0; i < n; ++i) {
        const int rc = validate(&ps[i], M[i], K[i]);
        if (rc) return rc;
        S2V_REQUIRE(ps[i].prec == ps[0].prec, "conv2d_group: members of one precision");
    }
    const int cus = plan_cus();
    double best = 1e30;
    gp.cfg = -1;
    for (int cfg : group_tiles()) {
        bool ok = true;
        for (int i = 0; i < n && ok; ++i) ok = group_member_ok(&ps[i], cfg) &&
                                              (long long)cdiv(ps[i].cout, kX3Tiles[cfg].t.bn) * kX3Tiles[cfg].t.bn <= ps[i].npad;
        if (!ok) continue;
        const X3Cfg &c = kX3Tiles[cfg];
        const double lat = c.t.nw == 4 ? 0.5e-6 : 0.6e-6;
        const double slots = (double)cus * c.bpc;
        int s[kPlanGroupMax] = {1, 1, 1, 1};
        long long tiles[kPlanGroupMax];
        for (int i = 0; i < n; ++i) tiles[i] = (long long)cdiv(M[i], c.t.bm) * cdiv(ps[i].cout, c.t.bn);
        int combos = 1;
        for (int i = 0; i < n; ++i) combos *= 5;
        for (int cb = 0; cb < combos; ++cb) {
            int v = cb;
            long long blocks = 0;
            int maxtps = 0;
            double red = 0.0;
            bool any_split = false, bad = false;
            for (int i = 0; i < n; ++i) {
                s[i] = 1 << (v % 5);
                v /= 5;
                const int kt = (K[i] + 31) / 32;
                if (s[i] > 1 && s[i] > kt / 4) { bad = true; break; }
                const int tps = (kt + s[i] - 1) / s[i];
                blocks += tiles[i] * s[i];
                maxtps = tps > maxtps ? tps : maxtps;
                if (s[i] > 1) {
                    any_split = true;
                    red += (double)M[i] * ps[i].cout * 4.0 * (s[i] + 1) / 4e12;
                }
            }
            if (bad) continue;
            const double conc = blocks < slots ? (double)blocks : slots;
            const double thr = 2.0 * c.t.bm * c.t.bn * 32.0 / (c.tflops * 1e12 / (conc > cus ? conc : cus));
            const double rounds = std::ceil((double)blocks / slots);
            double t = rounds * (2e-6 + maxtps * (thr > lat ? thr : lat));
            if (any_split) t += 7e-6 + red;
            if (t < best * 0.97) {
                best = t;
                gp.cfg = cfg;
                for (int i = 0; i < n; ++i) splits[i] = s[i];
            }
        }
    }
    S2V_REQUIRE(gp.cfg >= 0, "conv2d_group: members need the split-precision buffer-load path (direct zero-padded "
                "conv, cin %% 32 == 0, <= 32 taps, no in_scale / pre_act / pool / grid_cap / force_tile / post / dup, batch 1)");
    gp.ws_bytes = 0;
    for (int i = 0; i < n; ++i) {
        Plan &pl = gp.plan[i];
        pl = new_plan(&ps[i], M[i], K[i]);
        finish_x3(&ps[i], pl, gp.cfg, splits[i]);
        // each member's partial sums: a 256-byte aligned slice of member 0's workspace
        gp.ws_off[i] = gp.ws_bytes;
        if (pl.splits > 1) gp.ws_bytes += ((size_t)pl.splits * M[i] * ps[i].cout * sizeof(float) + 255) / 256 * 256;
    }
    return 0;
}

}  // namespace s2v
