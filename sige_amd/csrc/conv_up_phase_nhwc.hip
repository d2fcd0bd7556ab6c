// Nearest-x2 Upsample conv as four 2x2 phase convs on the half-resolution tensor (conv_mfma.hpp: the PH form of the body), NHWC,
// exact fp32, raw gather into a full tensor: explicit instantiations of the block shapes the Upsample launches use.
#include "conv_mfma.hpp"
namespace sige {
using G16 = ConvGeo<2, 1, 3, 16>;
using G32 = ConvGeo<2, 1, 3, 32>;
SIGE_CONV_PHASE_INSTANTIATE(G16, 1)
SIGE_CONV_PHASE_INSTANTIATE(G16, 2)
SIGE_CONV_PHASE_INSTANTIATE(G32, 1)
}  // namespace sige
