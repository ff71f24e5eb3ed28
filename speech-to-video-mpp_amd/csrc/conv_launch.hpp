// One launch function per convolution kernel family: declared here, defined next to the kernels,
// called by the entry points in conv.hip with the parameters the planner chose (conv_plan.hpp).
#pragma once
#include "conv_impl.hpp"

namespace s2v {

template <int ELT>   // 0 = bf16, 1 = f16 halves, 2 = single-pass f16 (conv_x3_impl.hpp; instances in conv_x3_{bf16,f16,f16s}.hip); 0 or an error
int launch_conv_x3(int tile, const ConvArgs &a, int amode, bool bkn, dim3 grid, hipStream_t s);
template <int ELT>   // LDS-DMA kernels on split-layout inputs (conv_glds.hip): cfg 0 = 256x256, 1 = 256x128, 2 = 512x128
void launch_conv_glds(int cfg, const ConvArgs &a, dim3 grid, hipStream_t s);
template <int ELT>   // grouped x3 launches (conv_x3_impl.hpp conv_igemm_x3_group): 0 or an error
int launch_conv_x3_group(int cfg, const ConvGroup &g, dim3 grid, hipStream_t s);
template <int ELT>   // narrow-N register-direct-A kernel (conv_x3_nar.hip); breg: B fragments direct too
int launch_conv_x3_nar(const ConvArgs &a, bool breg, dim3 grid, hipStream_t s);
template <int ELT>   // 3x3 spatial-patch kernel with the input halo staged once per channel slice (conv_x3_halo_impl.hpp; ELT 0..2)
int launch_conv_x3_halo(const ConvArgs &a, int th, int wn, dim3 grid, hipStream_t s);

// split-precision Cout <= 4 heads (conv_head.hip): 0 or an error
int launch_conv_head_x3(const ConvArgs &a, int prec, int co, int ks, int ncs, int th, hipStream_t s);
// 4-channel 1x1 / 3x3 convs on the exact-fp32 MFMA (conv_k4.hip): 0 or an error
int launch_conv_k4(const ConvArgs &a, int batch, int kt, hipStream_t s);

// fp32 VALU kernels (conv_valu.hip)
// conv_smallk4<qpt, kt> (kt 1 / 9) or conv_smallk<qpt, 1> (kt 0): tppx threads per pixel, iters groups per block
void launch_conv_smallk(const ConvArgs &a, int batch, int tppx, int qpt, int kt, int iters, int vec, hipStream_t s);
// conv_small_cpar<cout, lanes, lds_w>, or conv_direct_small<cout> when lanes == 0
void launch_conv_small(const ConvArgs &a, int batch, int lanes, bool lds_w, hipStream_t s);
// conv_halo_small<cout, ks> over 8 x 128 output tiles x a.splits channel ranges
void launch_conv_halo_small(const ConvArgs &a, int ks, hipStream_t s);

}  // namespace s2v
