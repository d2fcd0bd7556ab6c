// conv_tile3.hpp instantiated over 10x10 windows (block size 10): exact fp32, one window = 8x8 = 64 output pixels x 64 output
// channels per workgroup.  Gather: raw | cached affine (+ SiLU), one tensor | a fused cat; scatter_gather: raw.
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): 202 (gather, raw) / 210 (cat) / 214-218 (affine) / 240 (scatter_gather)
// VGPRs, no AGPRs, no spills, 69 632 B of LDS -- two workgroups per CU by registers (<= 256) and by LDS alike, which is what
// __launch_bounds__(256, OCC = 2) asks for; three would need <= 168 registers and 53 KB.
// Measured (profiles/block10_bench.json, launch by launch, weights L2-warm): at a 15 % edit 99-114 TFLOP/s on gather + affine + SiLU ->
// tiles against 79-89 for the 6x6 list on the kernel the router picks; at 5 % 76 against 61 (256^2, 192 workgroups) and 55 against
// 64 (128^2 / 256 channels: 120 workgroups do not fill 256 CUs).
#include "conv_tile3.hpp"
namespace sige {
using G10 = Tile3GeoE10;
void launch_conv_tile3_b10_gather(const Tile3Args &a, bool aff, bool cat, bool full, hipStream_t st) {
    const dim3 grid(a.T * a.ntn);
#define SIGE_T3(AFF, CAT)                                                                                      \
    do {                                                                                                       \
        if (full) conv_tile3_kernel<G10, T3_GATHER, AFF, CAT, true><<<grid, 256, 0, st>>>(a);                  \
        else conv_tile3_kernel<G10, T3_GATHER, AFF, CAT, false><<<grid, 256, 0, st>>>(a);                      \
    } while (0)
    if (aff && cat) SIGE_T3(true, true);
    else if (aff) SIGE_T3(true, false);
    else if (cat) SIGE_T3(false, true);
    else SIGE_T3(false, false);
#undef SIGE_T3
}
void launch_conv_tile3_b10_sg(const Tile3Args &a, bool full, hipStream_t st) {
    const dim3 grid(a.T * a.ntn);
    if (full) conv_tile3_kernel<G10, T3_SCATTER_GATHER, false, false, true><<<grid, 256, 0, st>>>(a);
    else conv_tile3_kernel<G10, T3_SCATTER_GATHER, false, false, false><<<grid, 256, 0, st>>>(a);
}
}  // namespace sige
