// bf16 / f16 split-precision instances of the halo-staged 3x3 convolution (conv_x3_halo_impl.hpp).
#include "conv_x3_halo_impl.hpp"

namespace s2v {
template int launch_conv_x3_halo<0>(const ConvArgs &, int, int, dim3, hipStream_t);
template int launch_conv_x3_halo<1>(const ConvArgs &, int, int, dim3, hipStream_t);
}  // namespace s2v
