// The convolution planner (conv_plan.cpp, host only): which kernel instance runs an s2v_conv_params
// launch, with which grid parameters and how much workspace.  plan_conv() fills one Plan; the entry
// points (conv.hip) encode it (s2v_conv2d_plan), report its workspace (s2v_conv2d_ws_bytes) and
// launch from it (s2v_conv2d) without deciding anything again.
#pragma once
#include <cstddef>

#include "host.hpp"

namespace s2v {

// One value per kernel family.
enum class Route {
    Glds,          // conv_glds_x3 (conv_glds.hip): LDS-DMA tiles on split-layout inputs
    HeadX3,        // conv_head_x3 (conv_head.hip): split-precision Cout <= 4 heads, 5x5 / 7x7
    HaloSmall,     // conv_halo_small (conv_valu.hip): fp32 Cout <= 4 heads with a staged input halo
    SmallCpar,     // conv_small_cpar (conv_valu.hip): Cout <= 4, lanes split the channels of a pixel
    DirectSmall,   // conv_direct_small (conv_valu.hip): Cout <= 4, one thread per pixel
    K4,            // conv_k4_mfma (conv_k4.hip): 4-channel inputs on the exact-fp32 MFMA
    SmallK,        // conv_smallk (conv_valu.hip): K <= 64
    SmallK4,       // conv_smallk4 (conv_valu.hip): 4-channel 1x1 / 3x3 inputs
    X3Tile,        // conv_igemm_x3 / conv_igemm_x3_persist (conv_x3_impl.hpp): split-precision tiles
    X3Nar,         // conv_x3_nar (conv_x3_nar.hip)
    X3Halo,        // conv_x3_halo (conv_x3_halo.hip)
    Igemm          // conv_igemm (conv.hip): fp32 MFMA tiles
};

struct TileCfg {
    int bm, bn, wm, nw, ks, pf;   // nw / ks / pf: waves, K-slices per stage (Glds: LDS stages), prefetch sets
};

struct Plan {
    Route route;
    int M, K, batch;         // GEMM rows / depth of one batch entry, batch entries (>= 1)
    int cout, prec;
    bool bkn;
    int tile;                // index into the route's table (kGlds / kX3Tiles / kTiles); 0 on the other routes
    TileCfg t;               // that table entry (tile routes)
    int splits, tps, ktiles;
    int kslab;               // split-K granularity in K-slices (9 for conv_x3_halo: whole channel slices)
    int amode;               // A-operand mode of the X3Tile / Igemm kernels
    int persist;             // X3Tile: persistent blocks under grid_cap, 0 = one block per tile
    int tppx, qpt, kt, iters;   // SmallK / SmallK4: threads per pixel, quads per thread, taps (0: runtime), groups
                                // per block / (256 / tppx); kt also K4's tap count
    int lanes;               // SmallCpar: lanes per output pixel
    bool lds_w;              // SmallCpar: the filter is staged in LDS
    int fsize;               // HaloSmall / HeadX3: filter size
    int ncs, rows;           // HeadX3: 32-channel slices per group (1 / 2), output rows per block
    int th, wn;              // X3Halo: patch rows, 64-channel wave columns
    unsigned x_bytes, w_bytes;   // buffer-load extents (AMODE 4, X3Nar, X3Halo), else 0
    size_t ws_bytes;         // split workspace the launch needs (0: none)
};

constexpr int kPlanGroupMax = 4;      // == kConvGroupMax (conv_impl.hpp)
struct GroupPlan {
    int cfg;                          // kX3Tiles index every member runs on
    Plan plan[kPlanGroupMax];
    size_t ws_off[kPlanGroupMax];     // member i's slice of member 0's workspace (members with splits > 1)
    size_t ws_bytes;
};

// true for the routes whose kernels read the split (wt_x3) weights of this launch
inline bool is_x3(const Plan &pl) {
    return pl.route == Route::X3Tile || pl.route == Route::X3Nar || pl.route == Route::X3Halo;
}
inline bool reads_wt_x3(const Plan &pl) {
    return pl.route == Route::Glds || pl.route == Route::HeadX3 || (!pl.bkn && is_x3(pl));
}

// Blocks of the split-K fold over ``rows`` output rows: one thread per channel quad when cout % 4 == 0.
inline long long fold_blocks(long long rows, int cout, long long cap) {
    const long long blocks = (rows * (cout % 4 == 0 ? cout / 4 : cout) + 255) / 256;
    return blocks < cap ? blocks : cap;
}

int plan_conv(const s2v_conv_params *p, Plan &pl);                   // validate + plan: 0 or an error
int plan_group(const s2v_conv_params *ps, int n, GroupPlan &gp);     // s2v_conv2d_group's members
void encode_plan(const Plan &pl, int *out11);                        // the eleven ints of s2v_conv2d_plan
int epi_vec4(const s2v_conv_params *p);                              // 16-byte epilogue stores are possible
long long tune_set(int key, long long value);                        // s2v_tune: returns the previous value

}  // namespace s2v
