// Single-pass f16 instances (S2V_PREC_F16, ELT 2) of the split-fp32 implicit-GEMM convolution
// (conv_x3_impl.hpp): the plain, persistent and grouped forms.
#include "conv_x3_impl.hpp"

#include "conv_launch.hpp"

namespace s2v {
extern template bool launch_conv_x3_part<2, 1>(int, const ConvArgs &, int, bool, dim3, hipStream_t);
extern template bool launch_conv_x3_part<2, 2>(int, const ConvArgs &, int, bool, dim3, hipStream_t);
template bool launch_conv_x3_part<2, 0>(int, const ConvArgs &, int, bool, dim3, hipStream_t);
template int launch_conv_x3<2>(int cfg, const ConvArgs &a, int amode, bool bkn, dim3 grid, hipStream_t s);
template int launch_conv_x3_group<2>(int cfg, const ConvGroup &g, dim3 grid, hipStream_t s);
}  // namespace s2v
