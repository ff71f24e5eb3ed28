// Implicit-GEMM convolution / GEMM on gfx950 fp32 MFMA (v_mfma_f32_32x32x2_f32).
//
// GEMM view:  M = batch pixels (n, oy, ox)   N = output channels   K = (ky, kx, cin)
//   A[m][k]  gathered on the fly from the NHWC input (zero / reflect padding, nearest-x2
//            upsampling, transposed-conv scatter-as-gather), prologue act/in_scale fused;
//   B[n][k]  pre-packed weights [npad][kpad] (or an activation matrix [K][N], ``b_kn``);
//   C        NHWC output slice; epilogue fuses bias/BN/demod scale, noise, residual, act.
//
// Block = 256 threads = 4 waves laid out WAVES_M x WAVES_N; each wave owns a
// (BM/WAVES_M) x (BN/WAVES_N) sub-tile made of 32x32 MFMA tiles. K is staged through LDS in
// BK = 32 slices held K-contiguous ([row][BK+4] floats; the +4 pad makes the ds_read_b128 of 16
// consecutive rows conflict-free), so each lane feeds 4 MFMA k-steps from one 16-byte read.
// Global loads of slice t+1 are issued into registers before the MFMAs of slice t (one LDS
// buffer, register double-buffering).  Split-K writes raw partial sums to a workspace that
// ``splitk_reduce`` folds with the same epilogue.
//
// This file: the fp32 tile kernel, the split-K folds and the extern "C" entry points.  The planner (conv_plan.cpp)
// decides the kernel family and every instance parameter, once; the other families sit behind conv_launch.hpp.
#include "conv_store4.hpp"

#include "conv_launch.hpp"
#include "conv_plan.hpp"

namespace s2v {

static_assert(kPlanGroupMax == kConvGroupMax, "the planner's group size is the kernels'");

template <int BM, int BN, int AR, int BR, int BKN>
__device__ __forceinline__ void store_ab(float *As, float *Bs, int tid, const f4 (&ra)[AR],
                                         const f4 (&rb)[BR]) {
    constexpr int LDK = 36;
    const int ar = tid >> 3, ak = (tid & 7) * 4;
#pragma unroll
    for (int j = 0; j < AR; ++j) *(f4 *)&As[(ar + 32 * j) * LDK + ak] = ra[j];
    if (!BKN) {
#pragma unroll
        for (int j = 0; j < BR; ++j) *(f4 *)&Bs[(ar + 32 * j) * LDK + ak] = rb[j];
    } else {
        constexpr int NV = BN / 4, RPP = 256 / NV;
        const int kr = tid / NV, nn = (tid - (tid / NV) * NV) * 4;
#pragma unroll
        for (int j = 0; j < BR; ++j) {
            const int k = kr + RPP * j;
            Bs[(nn + 0) * LDK + k] = rb[j].x;
            Bs[(nn + 1) * LDK + k] = rb[j].y;
            Bs[(nn + 2) * LDK + k] = rb[j].z;
            Bs[(nn + 3) * LDK + k] = rb[j].w;
        }
    }
}

template <int BM, int BN, int WAVES_M, int AMODE, int BKN>
__global__ __launch_bounds__(256, 1) void conv_igemm(ConvArgs a) {
    constexpr int BK = 32, LDK = BK + 4;
    constexpr int WAVES_N = 4 / WAVES_M;
    constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int AR = BM / 32;
    constexpr int BR = BN / 32;
    constexpr int STAGE = (BM + BN) * LDK;
    static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "tile");
    launch_stamp(a, false);

    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    // XCD-aware tile order: the dispatcher deals workgroups round-robin over the 8 XCDs, so
    // remap the linear id so that each XCD owns a contiguous run of tiles (neighbouring output
    // rows share their 3x3 halo through that XCD's L2), N-tiles of one M-tile adjacent.
    int mt, nt, bz;
    {
        const int gx = gridDim.x, gy = gridDim.y;
        const int total = gx * gy * gridDim.z;
        const int L = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
        const int per = total >> 3, rem = total & 7;
        const int xcd = L & 7, idx = L >> 3;
        const int Lp = xcd < rem ? xcd * (per + 1) + idx : rem * (per + 1) + (xcd - rem) * per + idx;
        nt = Lp % gy;
        const int t = Lp / gy;
        mt = t % gx;
        bz = t / gx;
    }
    const int m0 = mt * BM, n0 = nt * BN;
    const int bidx = bz / a.splits, split = bz - bidx * a.splits;
    const float *__restrict__ x = a.x + (long long)bidx * a.x_bs;
    const float *__restrict__ wt = a.wt + (long long)bidx * a.w_bs;
    const int kt0 = split * a.tps;
    const int kt1 = min(a.ktiles, kt0 + a.tps);
    // AMODE 0/3: visit K-slices channel-slice-major (all taps of one 32-channel slice in a row),
    // so the 3x3 neighbourhood of a slice is re-read from L2 right away instead of after the
    // whole channel range; the weights are indexed by the same permuted slice, so the sum is
    // unchanged apart from fp32 summation order.
    const int taps = a.kh * a.kw, nsl = a.cin >> 5;
    const bool kperm = (AMODE == 0 || AMODE == 3) && !BKN && taps > 1;
    auto kmap = [&](int i) { return kperm ? (i % taps) * nsl + i / taps : i; };
    const int ar = tid >> 3, ak = (tid & 7) * 4;

    ARows<AR, AMODE> R;
    a_rows_init<AR, AMODE>(a, m0, ar, R);

    f4 ra[AR], rb[BR];
    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int li = lane & 31, lh = lane >> 5;
    if (kt0 < kt1) {
        load_a<AR, AMODE>(a, x, kmap(kt0), ak, R, ra);
        load_b<BN, BR, BKN>(a, wt, kmap(kt0), n0, tid, rb);
        store_ab<BM, BN, AR, BR, BKN>(smem, smem + BM * LDK, tid, ra, rb);
        __syncthreads();
    }
    int buf = 0;
    for (int kt = kt0; kt < kt1; ++kt) {
        // prefetch slice kt+1 into registers (the last iteration re-reads its own slice: no
        // control flow around the staging registers); it lands while the MFMAs below run
        const int kn = kmap(min(kt + 1, kt1 - 1));
        load_a<AR, AMODE>(a, x, kn, ak, R, ra);
        load_b<BN, BR, BKN>(a, wt, kn, n0, tid, rb);
        __builtin_amdgcn_sched_barrier(0);   // keep the prefetch issue above the MFMA block
        const float *As = smem + buf * STAGE;
        const float *Bs = As + BM * LDK;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f4 av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                av[i] = *(const f4 *)&As[(wm * WTM + i * 32 + li) * LDK + lh * 16 + q * 4];
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bv[j] = *(const f4 *)&Bs[(wn * WTN + j * 32 + li) * LDK + lh * 16 + q * 4];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].x, bv[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].y, bv[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].z, bv[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].w, bv[j].w, acc[i][j], 0, 0, 0);
                }
        }
        // the other buffer was last read before the previous barrier
        float *Ad = smem + (buf ^ 1) * STAGE;
        store_ab<BM, BN, AR, BR, BKN>(Ad, Ad + BM * LDK, tid, ra, rb);
        __syncthreads();
        buf ^= 1;
    }

    // ---- epilogue (shared with the split-bf16 kernel, conv_impl.hpp)
    static_assert(BM * (BN + 4) <= 2 * STAGE, "C tile must fit in the staging LDS");
    epilogue_tile<BM, BN, WAVES_M, TM, TN>(a, acc, smem, tid, m0, n0, bz, bidx);
    launch_stamp(a, true);
}

// Split-K fold: one thread per 4 consecutive output channels (16-byte partial-sum loads) when
// cout % 4 == 0, else per channel; the epilogue is the kernels' own (one 16-byte store when ``vec``).
// 32-bit index math when the fold has < 2^31 items (the 64-bit divisions cost more VALU than the
// fold's arithmetic).

__global__ void splitk_reduce(ConvArgs a, int batch, int vec) {
    const int cv = (a.cout & 3) == 0 ? 4 : 1;
    const int nq = a.cout / cv;
    const long long total = (long long)batch * a.M * nq;
    const long long slab = (long long)a.M * a.cout;
    const bool small = total < (1LL << 31);
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        int q, m, bidx;
        if (small) {
            const unsigned u = (unsigned)idx, bm = u / (unsigned)nq;
            q = (int)(u - bm * (unsigned)nq);
            bidx = (int)(bm / (unsigned)a.M);
            m = (int)(bm - (unsigned)bidx * (unsigned)a.M);
        } else {
            q = (int)(idx % nq);
            const long long bm = idx / nq;
            m = (int)(bm % a.M);
            bidx = (int)(bm / a.M);
        }
        const float *src = a.ws + (long long)bidx * a.splits * slab + (long long)m * a.cout + q * cv;
        if (cv == 4) {
            f4 s = *(const f4 *)src;
            for (int sp = 1; sp < a.splits; ++sp) s += *(const f4 *)(src + sp * slab);
            store_epilogue4(a, bidx, m, 4 * q, s, vec != 0, false);
        } else {
            float s = src[0];
            for (int sp = 1; sp < a.splits; ++sp) s += src[sp * slab];
            store_epilogue(a, bidx, m, q, s);
        }
    }
}

// Split-K fold of a conv group (s2v_conv2d_group): member p folds with the blocks
// [rstart[p], rstart[p + 1]) (none when it has one split), otherwise as splitk_reduce.
__global__ void splitk_reduce_group(ConvGroup g) {
    int p = 0;
#pragma unroll
    for (int i = 1; i < kConvGroupMax; ++i)
        if (i < g.n && (int)blockIdx.x >= g.rstart[i]) p = i;
    const ConvArgs &a = g.a[p];
    const int nb = g.rstart[p + 1] - g.rstart[p];
    const int cv = (a.cout & 3) == 0 ? 4 : 1;
    const int nq = a.cout / cv;
    const long long total = (long long)a.M * nq;               // one batch entry (group members: batch 1)
    const long long slab = (long long)a.M * a.cout;
    for (long long idx = (blockIdx.x - g.rstart[p]) * (long long)blockDim.x + threadIdx.x; idx < total;
         idx += (long long)nb * blockDim.x) {
        const unsigned u = (unsigned)idx;
        const int m = (int)(u / (unsigned)nq), q = (int)(u - (unsigned)m * (unsigned)nq);
        const float *src = a.ws + (long long)m * a.cout + q * cv;
        if (cv == 4) {
            f4 sum = *(const f4 *)src;
            for (int sp = 1; sp < a.splits; ++sp) sum += *(const f4 *)(src + sp * slab);
            store_epilogue4(a, 0, m, 4 * q, sum, g.vec[p] != 0, false);
        } else {
            float sum = src[0];
            for (int sp = 1; sp < a.splits; ++sp) sum += src[sp * slab];
            store_epilogue(a, 0, m, q, sum);
        }
    }
}

static ConvArgs make_args(const s2v_conv_params *p, const Plan &pl) {
    ConvArgs a{};
    a.x = p->x; a.n = p->n; a.h = p->h; a.w = p->w; a.cin = p->cin; a.xcs = p->xcs;
    a.in_mode = p->in_mode; a.pad_mode = p->pad_mode; a.pre_act = p->pre_act; a.pre_alpha = p->pre_alpha;
    a.in_scale = p->in_scale; a.in_scale_ns = p->in_scale_ns;
    a.kh = p->kh; a.kw = p->kw; a.sh = p->sh; a.sw = p->sw; a.ph = p->ph; a.pw = p->pw; a.dh = p->dh; a.dw = p->dw;
    a.wt = reads_wt_x3(pl) ? (const float *)p->wt_x3 : p->wt;
    a.kpad = p->kpad; a.cout = p->cout; a.ldb = p->ldb;
    a.y = p->y; a.oh = p->oh; a.ow = p->ow; a.ycs = p->ycs;
    Epi &e = a.epi;
    e.scale = p->scale; e.shift = p->shift; e.nc_scale = p->nc_scale; e.nc_ns = p->nc_scale_ns;
    e.pix_add = p->pix_add; e.pix_w = p->pix_w; e.res = p->res; e.res_cs = p->res_cs;
    e.res_h = p->res_h > 0 ? p->res_h : p->oh; e.res_w = p->res_w > 0 ? p->res_w : p->ow;
    e.res_oy = p->res_oy; e.res_ox = p->res_ox; e.res_after = p->res_after_act;
    e.res_simple = (e.res_h == p->oh && e.res_w == p->ow && p->res_oy == 0 && p->res_ox == 0);
    e.act = p->act; e.alpha = p->alpha;
    e.post_mul = p->post_mul; e.post_add = p->post_add; e.post_cs = p->post_cs; e.post_c0 = p->post_c0;
    e.dup_src = p->dup_src; e.dup_bias = p->dup_bias; e.dup_a = p->dup_a; e.dup_cs = p->dup_cs; e.dup_off = p->dup_off;
    a.x_bs = p->x_bs; a.w_bs = p->w_bs; a.y_bs = p->y_bs; a.res_bs = p->res_bs;
    a.M = pl.M; a.K = pl.K; a.ktiles = pl.ktiles; a.splits = pl.splits; a.tps = pl.tps; a.ws = p->ws;
    a.x_bytes = pl.x_bytes; a.w_bytes = pl.w_bytes;
    a.y_step = p->out_step > 1 ? p->out_step : 1; a.y_h = p->out_full_h; a.y_w = p->out_full_w;
    a.d2s_c = p->d2s_cout > 0 ? p->d2s_cout : 0;
    // the split weights' pre-scale and the A operand's pre-scale leave through the accumulator factor
    a.acc_scale = (reads_wt_x3(pl) && p->wt_scale > 0.f) ? 1.f / p->wt_scale : 1.f;
    a.pool = p->out_pool != 0;
    a.stamps = p->stamps; a.stamp_ctr = p->stamp_ctr; a.stamp_slot = p->stamp_slot;
    a.stamp_stride = p->stamp_stride; a.stamp_reps = p->stamp_reps > 0 ? p->stamp_reps : 1;
    a.x_scale = 1.f;
    a.nonfinite = p->nonfinite;
    static const bool vec4_on = [] { const char *e = getenv("S2V_EPI_VEC4"); return !e || atoi(e) != 0; }();
    a.vec4 = vec4_on && epi_vec4(p) && (!p->nc_scale || (p->nc_scale_ns % 4 == 0 && ((uintptr_t)p->nc_scale % 16) == 0)) &&
             (p->d2s_cout <= 0 || p->d2s_cout % 4 == 0);
    if (reads_wt_x3(pl) && pl.route != Route::Glds && p->x_scale > 0.f && p->x_scale != 1.f) {
        a.x_scale = p->x_scale;
        a.acc_scale /= p->x_scale;
    }
    return a;
}

template <int BM, int BN, int WM>
static void launch_tile(const ConvArgs &a, int amode, bool bkn, dim3 grid, hipStream_t s) {
    switch (amode * 2 + (bkn ? 1 : 0)) {
        case 0: conv_igemm<BM, BN, WM, 0, 0><<<grid, 256, 0, s>>>(a); break;
        case 1: conv_igemm<BM, BN, WM, 0, 1><<<grid, 256, 0, s>>>(a); break;
        case 2: conv_igemm<BM, BN, WM, 1, 0><<<grid, 256, 0, s>>>(a); break;
        case 3: conv_igemm<BM, BN, WM, 1, 1><<<grid, 256, 0, s>>>(a); break;
        case 4: conv_igemm<BM, BN, WM, 2, 0><<<grid, 256, 0, s>>>(a); break;
        case 5: conv_igemm<BM, BN, WM, 2, 1><<<grid, 256, 0, s>>>(a); break;
        default: conv_igemm<BM, BN, WM, 3, 0><<<grid, 256, 0, s>>>(a); break;   // 6 (reflect, packed B)
    }
}

static void launch_igemm(int tile, const ConvArgs &a, int amode, bool bkn, dim3 grid, hipStream_t s) {
    switch (tile) {
        case 0: launch_tile<128, 128, 2>(a, amode, bkn, grid, s); break;
        case 1: launch_tile<128, 64, 2>(a, amode, bkn, grid, s); break;
        case 2: launch_tile<64, 128, 2>(a, amode, bkn, grid, s); break;
        case 3: launch_tile<64, 64, 2>(a, amode, bkn, grid, s); break;
        case 4: launch_tile<256, 32, 4>(a, amode, bkn, grid, s); break;
        default: launch_tile<128, 32, 4>(a, amode, bkn, grid, s); break;
    }
}

}  // namespace s2v

using namespace s2v;

extern "C" size_t s2v_conv2d_group_ws_bytes(const s2v_conv_params *ps, int n) {
    GroupPlan gp;
    return plan_group(ps, n, gp) ? 0 : gp.ws_bytes;
}

extern "C" int s2v_conv2d_group_plan(const s2v_conv_params *ps, int n, int *out) {
    GroupPlan gp;
    const int rc = plan_group(ps, n, gp);
    if (rc) return rc;
    out[0] = gp.cfg;
    for (int i = 0; i < n; ++i) out[1 + i] = gp.plan[i].splits;
    return 0;
}

extern "C" int s2v_conv2d_group(const s2v_conv_params *ps, int n, s2v_stream_t stream) {
    GroupPlan gp;
    int rc = plan_group(ps, n, gp);
    if (rc) return rc;
    if (gp.ws_bytes && (!ps[0].ws || ps[0].ws_bytes < gp.ws_bytes)) {
        set_error("conv2d_group: split-K workspace of %zu bytes required in member 0 (have %zu)", gp.ws_bytes, ps[0].ws_bytes);
        return S2V_E_WORKSPACE;
    }
    ConvGroup g{};
    g.n = n;
    long long blocks = 0, rblocks = 0;
    for (int i = 0; i < n; ++i) {
        const Plan &pl = gp.plan[i];
        ConvArgs &a = g.a[i];
        a = make_args(&ps[i], pl);
        a.stamps = nullptr;
        if (pl.splits > 1) a.ws = (float *)((char *)ps[0].ws + gp.ws_off[i]);
        g.gx[i] = (int)cdiv(pl.M, pl.t.bm);
        g.gy[i] = (int)cdiv(pl.cout, pl.t.bn);
        g.start[i] = (int)blocks;
        blocks += (long long)g.gx[i] * g.gy[i] * pl.splits;
        g.rstart[i] = (int)rblocks;
        if (pl.splits > 1) rblocks += fold_blocks(pl.M, pl.cout, 1024);
        g.vec[i] = epi_vec4(&ps[i]);
    }
    for (int i = n; i <= kConvGroupMax; ++i) {
        g.start[i] = (int)blocks;
        g.rstart[i] = (int)rblocks;
    }
    S2V_REQUIRE(blocks < (1LL << 31), "conv2d_group: too many tiles");
    hipStream_t s = (hipStream_t)stream;
    // (a group runs the tile kernels only, so S2V_PREC_F16 members all run single-pass: gp.plan[].prec == 3)
    rc = ps[0].prec == S2V_PREC_BF16X3 ? launch_conv_x3_group<0>(gp.cfg, g, dim3((unsigned)blocks), s)
         : ps[0].prec == S2V_PREC_F16  ? launch_conv_x3_group<2>(gp.cfg, g, dim3((unsigned)blocks), s)
                                       : launch_conv_x3_group<1>(gp.cfg, g, dim3((unsigned)blocks), s);
    if (rc) return rc;
    rc = check_launch("conv2d_group");
    if (rc || rblocks == 0) return rc;
    splitk_reduce_group<<<(unsigned)rblocks, 256, 0, s>>>(g);
    return check_launch("splitk_reduce_group");
}

extern "C" int s2v_tune(int key, long long value, long long *old_value) {
    S2V_REQUIRE(key >= 0 && key < S2V_TUNE_COUNT, "tune: bad key %d", key);
    const long long prev = tune_set(key, value);
    if (old_value) *old_value = prev;
    return 0;
}

extern "C" size_t s2v_conv2d_ws_bytes(const s2v_conv_params *p) {
    Plan pl;
    return plan_conv(p, pl) ? 0 : pl.ws_bytes;
}

extern "C" int s2v_conv2d_plan(const s2v_conv_params *p, int *out11) {
    for (int i = 6; i < 11; ++i) out11[i] = 0;
    Plan pl;
    const int rc = plan_conv(p, pl);
    if (rc) return rc;
    encode_plan(pl, out11);
    return 0;
}

extern "C" int s2v_conv2d(const s2v_conv_params *p, s2v_stream_t stream) {
    Plan pl;
    int rc = plan_conv(p, pl);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool tiles = pl.route == Route::Glds || pl.route == Route::Igemm || is_x3(pl);
    if (pl.ws_bytes && (!p->ws || p->ws_bytes < pl.ws_bytes)) {
        set_error("conv2d: split%s workspace of %zu bytes required (have %zu)", tiles ? "-K" : "", pl.ws_bytes, p->ws_bytes);
        return S2V_E_WORKSPACE;
    }
    const ConvArgs a = make_args(p, pl);
    // pl.prec is the arithmetic the launch really runs: S2V_PREC_F16 on the tile / halo routes, S2V_PREC_F16X3
    // where that mode falls back (conv_plan.cpp make_plan)
    const bool bf16 = pl.prec == S2V_PREC_BF16X3, f16s = pl.prec == S2V_PREC_F16;
    dim3 grid;
    if (tiles) grid = dim3(cdiv(pl.M, pl.t.bm), cdiv(pl.cout, pl.t.bn), pl.batch * pl.splits);
    const char *what = "conv_igemm";
    switch (pl.route) {
        case Route::K4:
            rc = launch_conv_k4(a, pl.batch, pl.kt, s);
            what = "conv_k4";
            break;
        case Route::SmallK:
        case Route::SmallK4:
            launch_conv_smallk(a, pl.batch, pl.tppx, pl.qpt, pl.kt, pl.iters, epi_vec4(p), s);
            what = "conv_smallk";
            break;
        case Route::HeadX3:
            rc = launch_conv_head_x3(a, pl.prec, p->cout, pl.fsize, pl.ncs, pl.rows, s);
            what = "conv_head_x3";
            break;
        case Route::HaloSmall:
            launch_conv_halo_small(a, pl.fsize, s);
            what = "conv_halo_small";
            break;
        case Route::SmallCpar:
        case Route::DirectSmall:
            S2V_REQUIRE(pl.route == Route::SmallCpar || p->w_bs == 0 || pl.batch == 1 || pl.M % 256 == 0,
                        "conv2d: per-batch weights on the LDS-staged small-Cout path need M %% 256 == 0");
            launch_conv_small(a, pl.batch, pl.lanes, pl.lds_w, s);
            what = "conv_small";
            break;
        case Route::Glds:
            if (bf16) launch_conv_glds<0>(pl.tile, a, grid, s);
            else launch_conv_glds<1>(pl.tile, a, grid, s);
            break;
        case Route::X3Halo:                       // one block per (image, patch)
            grid.x = (unsigned)((long long)p->n * cdiv(p->oh, pl.th) * cdiv(p->ow, 64));
            rc = bf16   ? launch_conv_x3_halo<0>(a, pl.th, pl.wn, grid, s)
                 : f16s ? launch_conv_x3_halo<2>(a, pl.th, pl.wn, grid, s)
                        : launch_conv_x3_halo<1>(a, pl.th, pl.wn, grid, s);
            break;
        case Route::X3Nar:
            rc = bf16 ? launch_conv_x3_nar<0>(a, pl.amode == 7, grid, s) : launch_conv_x3_nar<1>(a, pl.amode == 7, grid, s);
            break;
        case Route::X3Tile: {
            ConvArgs ap = a;
            if (pl.persist > 0) {                 // persistent blocks over the tile grid (s2v.h grid_cap)
                ap.vgrid_x = (int)grid.x;
                ap.vgrid_y = (int)grid.y;
                ap.vgrid_z = (int)grid.z;
                grid = dim3((unsigned)pl.persist, 1, 1);
            }
            rc = bf16   ? launch_conv_x3<0>(pl.tile, ap, pl.amode, pl.bkn, grid, s)
                 : f16s ? launch_conv_x3<2>(pl.tile, ap, pl.amode, pl.bkn, grid, s)
                        : launch_conv_x3<1>(pl.tile, ap, pl.amode, pl.bkn, grid, s);
            break;
        }
        case Route::Igemm:
            launch_igemm(pl.tile, a, pl.amode, pl.bkn, grid, s);
            break;
    }
    if (rc) return rc;
    rc = check_launch(what);
    if (rc || pl.splits <= 1) return rc;
    // the shared split-K fold (the VALU head routes keep their one-thread-per-channel grid)
    const unsigned blocks = tiles ? (unsigned)fold_blocks((long long)pl.batch * pl.M, pl.cout, 65535LL * 4)
                                  : cdiv((long long)pl.M * pl.cout, 256);
    splitk_reduce<<<blocks, 256, 0, s>>>(a, pl.batch, epi_vec4(p));
    return check_launch("splitk_reduce");
}
