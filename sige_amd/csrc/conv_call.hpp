// One channels-last tile-conv call on the HOST: the record every extern "C" entry point of the tile convs fills from its raw
// arguments (behind its plan hook, which replays the entry point and so must see the raw arguments), and the checks those entry
// points share, each written once.  Everything between an entry point and a launch takes `const TileConvCall &`.  Plain C++, no
// HIP or kernel header: what a kernel receives (ConvArgs, Tile3Args, WideArgs) is filled from the record where it is launched.
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "sige_hip.h"

namespace sige {

enum { CALL_TILES = 0, CALL_GATHER = 1, CALL_SCATTER_GATHER = 2 };  // TileConvCall::source (1, 2 = the `source` of the v3 ABI)

struct StagingAffine {  // act(scale * x + shift) on the way into the conv; extents [scaleB, scaleC, 1, 1] as the caller gave them
    const float *scale, *shift;
    int scaleB, scaleC, shiftB, shiftC, act;
};

struct TwinOut {  // out = SiLU(scale * result + shift), written beside a full-tensor destination
    float *out;
    const float *scale, *shift;
};

// A zero-initialised record says "none of the optional groups": a tile slab in, tiles out, no affine, no epilogue.
struct TileConvCall {
    // ---- source: the tiles themselves, tiles gathered from x (| x2: a fused torch.cat), or x's tiles scattered over the cached x2
    int source;  // CALL_*
    const float *x;
    const void *x2;
    int x2_f16;              // x2 holds halves (fp16-stored caches)
    int B, C1, C2, H, W;     // (H, W): the size the tiles index -- with `up` the upsampled one
    int up;                  // 0 | 1 nearest x2 in the addressing | 2 the same as four phase convs
    int bH, bW;              // window
    const int32_t *idx;      // index list [N, 2]
    int N;
    const int32_t *map;      // scatter map; x's tiles are Rx x Sx
    int Rx, Sx;
    StagingAffine aff;
    // ---- weights: `packed` for conv_mfma.hpp; packed_tile3 = the v3 layout (conv_tile3.hpp), min_blocks = the router's threshold
    const float *packed, *bias, *packed_tile3;
    int Cout, kH, kW, strH, strW, min_blocks;
    // ---- destination: tiles, or the full tensor [B, Ho, Wo, Cout] at an offset, + residual (block residual: x1's tiles by table1)
    int to_full, offH, offW, Ho, Wo;
    const void *residual;
    int res_f16;
    const float *x1;
    const int32_t *table1;
    int gH1, gW1, N1, R1, S1;
    // ---- epilogue
    const float *oscale, *oshift;
    int oact;
    TwinOut twin[2];
    // ---- the rest: K-split workspace, output, stream
    float *ws;
    size_t ws_floats;
    float *out;
    void *stream;

    int Cin() const { return C1 + C2; }
    long tiles() const { return (long)B * N; }
};

// ---- the shared checks.  Where entry points answer one defect with different codes the caller names the code. ----
inline bool aligned16(std::initializer_list<const void *> ps) {
    uintptr_t bits = 0;
    for (const void *p : ps) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 15) == 0;
}
inline bool act_known(int act) { return act == SIGE_HIP_ACT_IDENTITY || act == SIGE_HIP_ACT_SWISH; }
inline bool offsets_fit(long elements) { return elements < (1L << 29); }  // 32-bit byte offsets in the kernels

// one operand of an affine broadcasts as [1|B, 1|C]
inline bool affine_extent_ok(const void *p, int b, int c, int B, int C) { return !p || ((b == 1 || b == B) && (c == 1 || c == C)); }

// scale and shift come as a pair with ONE broadcast shape; without them there is nothing to activate
inline int staging_affine_status(const StagingAffine &f, int B, int C, int pair_code, int extent_code) {
    if (!f.scale && !f.shift) return f.act == SIGE_HIP_ACT_IDENTITY ? SIGE_HIP_OK : SIGE_HIP_EUNSUPPORTED;
    if (!f.scale || !f.shift) return pair_code;
    if (f.scaleB != f.shiftB || f.scaleC != f.shiftC || !affine_extent_ok(f.scale, f.scaleB, f.scaleC, B, C)) return extent_code;
    return SIGE_HIP_OK;
}
inline int out_affine_status(const float *oscale, const float *oshift) {
    return (oscale == nullptr) != (oshift == nullptr) ? SIGE_HIP_EINVAL : SIGE_HIP_OK;
}
inline int twins_status(const TwinOut *t) {  // a twin comes with its scale and shift
    for (int k = 0; k < 2; ++k)
        if (t[k].out && !(t[k].scale && t[k].shift)) return SIGE_HIP_EINVAL;
    return SIGE_HIP_OK;
}
inline bool twins_aligned(const TwinOut *t) { return aligned16({t[0].out, t[1].out, t[0].scale, t[0].shift, t[1].scale, t[1].shift}); }

int stacked_shift(int H);  // (api.hip: sige_hip_set_edit_batch; log2 of one image's height, 0 = not stacked, < 0 = H does not stack)
inline int edit_shift_status(int H, int B, int *shift) {  // stacked edits stack along H of ONE image
    *shift = stacked_shift(H);
    return (*shift < 0 || (*shift && B != 1)) ? SIGE_HIP_EUNSUPPORTED : SIGE_HIP_OK;
}

}  // namespace sige
