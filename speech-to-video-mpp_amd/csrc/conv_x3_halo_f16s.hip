// Single-pass f16 instances (S2V_PREC_F16, ELT 2) of the halo-staged 3x3 convolution (conv_x3_halo_impl.hpp).
#include "conv_x3_halo_impl.hpp"

namespace s2v {
template int launch_conv_x3_halo<2>(const ConvArgs &, int, int, dim3, hipStream_t);
}  // namespace s2v
