// A 3x3 conv launch hosting a slice of a deferred 3x3 "side" conv (sige_hip_conv_side_begin): explicit instantiations of
// conv_side_kernel -- exact fp32, channels-last gather, destination = full tensor, 4 waves per workgroup; host 16 x 16 blocks,
// side conv 16 x 16 (NB 1) or 16 x 32 (NB 2) blocks.
#include "conv_mfma.hpp"
namespace sige {
using A16 = ConvGeo<3, 1, 6, 16>;
SIGE_CONV_SIDE_INSTANTIATE(A16, 1, A16, 1, DST_NCHW, 4)
SIGE_CONV_SIDE_INSTANTIATE(A16, 1, A16, 2, DST_NCHW, 4)
}  // namespace sige
