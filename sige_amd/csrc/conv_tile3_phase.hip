// conv_tile3.hpp instantiated over the four 2x2 phase convs of a nearest-x2 Upsample conv (Tile3GeoP): eight tiles x
// one phase x 64 output channels per workgroup, exact fp32 and fp16 operands; the pack of the phase kernels in the v3 stream order,
// and the C ABI.  Resources per instance (code-object metadata, gfx950): DESIGN.md 5.29.
#include "conv_call.hpp"
#include "conv_tile3.hpp"

namespace sige {

using GP8 = Tile3GeoP<8, WIDE_F32>;
using GP8H = Tile3GeoP<8, WIDE_F16>;

template <> void launch_conv_tile3_phase<8, WIDE_F32>(const Tile3Args &a, hipStream_t st) {
    conv_tile3_phase_kernel<GP8><<<dim3(ceil_div(a.T, GP8::TPW) * a.ntn, 4), 256, 0, st>>>(a);
}
template <> void launch_conv_tile3_phase<8, WIDE_F16>(const Tile3Args &a, hipStream_t st) {
    conv_tile3_phase_kernel<GP8H><<<dim3(ceil_div(a.T, GP8H::TPW) * a.ntn, 4), 256, 0, st>>>(a);
}

bool conv_side_armed();  // (block_conv.hip)
int flush_for_phase_tile3(const float *x, const float *residual, float *out, float *twin0, float *twin1, hipStream_t st);

// packed[phase][ntile][wave][chunk][tap = 2 kh + kw][nt][piece][lane = (kq, j)][e]: one phase's sub-pack is the stream
// sige_hip_wide_conv_pack lays out for a kernel of four taps, followed by kWidePadSteps steps of zeros of its own
//   exact fp32: e < 4, channel ci = 64 chunk + 16 wave + 2 (4 piece + e) + kq (conv_wide.hip: pack_wide_f32_kernel)
template <typename G>
__global__ void pack_phase3_f32_kernel(const float *__restrict__ w, int Cout, int Cin, float *__restrict__ packed, long per_phase, long sub_floats) {
    const int nchunks = Cin / G::CC;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < 4 * per_phase; i += (long)gridDim.x * blockDim.x) {
        const int ph = (int)(i / per_phase);
        long r = i - ph * per_phase;
        const long at = r;
        const int e = r % 4; r /= 4;
        const int j = r % 32; r /= 32;
        const int kq = r % 2; r /= 2;
        const int pl = r % 2; r /= 2;
        const int nt = r % 2; r /= 2;
        const int tap = r % G::KK; r /= G::KK;
        const int chunk = r % nchunks; r /= nchunks;
        const int wave = r % 4; r /= 4;
        const int ntile = (int)r;
        const int co = 64 * ntile + 32 * nt + j;
        const int ci = chunk * G::CC + wave * G::CW + 2 * (4 * pl + e) + kq;
        packed[ph * sub_floats + at] = w[(((size_t)ph * Cout + co) * Cin + ci) * G::KK + tap];
    }
}
//   fp16: e < 8, one piece, channel ci = 64 chunk + 16 wave + 8 kq + e, rounded RNE and saturated (pack_wide_kernel)
template <typename G>
__global__ void pack_phase3_f16_kernel(const float *__restrict__ w, int Cout, int Cin, _Float16 *__restrict__ packed, long per_phase, long sub_halves) {
    const int nchunks = Cin / G::CC;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < 4 * per_phase; i += (long)gridDim.x * blockDim.x) {
        const int ph = (int)(i / per_phase);
        long r = i - ph * per_phase;
        const long at = r;
        const int e = r % 8; r /= 8;
        const int j = r % 32; r /= 32;
        const int kq = r % 2; r /= 2;
        const int nt = r % 2; r /= 2;
        const int tap = r % G::KK; r /= G::KK;
        const int chunk = r % nchunks; r /= nchunks;
        const int wave = r % 4; r /= 4;
        const int ntile = (int)r;
        const int co = 64 * ntile + 32 * nt + j;
        const int ci = chunk * G::CC + wave * G::CW + 8 * kq + e;
        const float v = w[(((size_t)ph * Cout + co) * Cin + ci) * G::KK + tap];
        packed[ph * sub_halves + at] = (_Float16)fminf(fmaxf(v, -65504.0f), 65504.0f);
    }
}

}  // namespace sige

using namespace sige;

extern "C" int sige_hip_upsample_phase_tile3_supported(int C, int Cout) {
    return (C > 0 && C % 64 == 0 && Cout > 0 && Cout % 64 == 0) ? 1 : 0;
}

extern "C" size_t sige_hip_upsample_phase_tile3_packed_size(int Cout, int Cin, int prec) {
    if (!sige_hip_upsample_phase_tile3_supported(Cin, Cout) || (prec != WIDE_F32 && prec != WIDE_F16)) return 0;
    const long sub = prec == WIDE_F32 ? GP8::sub_bytes(Cout / 64, Cin / 64) : GP8H::sub_bytes(Cout / 64, Cin / 64);
    return (size_t)(4 * sub / 4);
}

extern "C" int sige_hip_upsample_phase_tile3_pack(const float *w_phases, int Cout, int Cin, int prec, float *packed, void *stream) {
    if (!w_phases || !packed || (prec != WIDE_F32 && prec != WIDE_F16)) return SIGE_HIP_EINVAL;
    if (!sige_hip_upsample_phase_tile3_supported(Cin, Cout)) return SIGE_HIP_EUNSUPPORTED;
    hipStream_t st = as_stream(stream);
    const size_t floats = sige_hip_upsample_phase_tile3_packed_size(Cout, Cin, prec);
    if (hipMemsetAsync(packed, 0, floats * 4, st) != hipSuccess) return SIGE_HIP_ELAUNCH;  // (incl. every sub-pack's padding)
    const int ntn = Cout / 64, nchunks = Cin / 64;
    if (prec == WIDE_F32) {
        const long sub = GP8::sub_bytes(ntn, nchunks) / 4, per_phase = sub - (long)kWidePadSteps * GP8::STEPB / 4;
        const int grid = (int)((4 * per_phase + 255) / 256 < 8192 ? (4 * per_phase + 255) / 256 : 8192);
        pack_phase3_f32_kernel<GP8><<<grid, 256, 0, st>>>(w_phases, Cout, Cin, packed, per_phase, sub);
    } else {
        const long sub = GP8H::sub_bytes(ntn, nchunks) / 2, per_phase = sub - (long)kWidePadSteps * GP8H::STEPB / 2;
        const int grid = (int)((4 * per_phase + 255) / 256 < 8192 ? (4 * per_phase + 255) / 256 : 8192);
        pack_phase3_f16_kernel<GP8H><<<grid, 256, 0, st>>>(w_phases, Cout, Cin, reinterpret_cast<_Float16 *>(packed), per_phase, sub);
    }
    return launch_status(1);
}

// This entry point has no launch-plan hook (as sige_hip_tile_conv3_block_nhwc): while a plan records it refuses, and the plan records
// the call the binding makes next.
extern "C" int sige_hip_upsample_phase_tile3_nhwc(
        int compute, const float *x, int B, int C, int H, int W, const int32_t *active_indices, int N,
        const float *packed_phase3, const float *bias, int Cout, int offsetH, int offsetW, const float *residual, int Ho, int Wo,
        const float *out_scale, const float *out_shift, int out_activation,
        float *twin0, const float *twin0_scale, const float *twin0_shift,
        float *twin1, const float *twin1_scale, const float *twin1_shift,
        int min_blocks, float *out, void *stream) {
    if (compute < 0 || compute > 2) return SIGE_HIP_EINVAL;
    if (B < 0 || N < 0 || C <= 0 || Cout <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return SIGE_HIP_EINVAL;
    if (compute == 2 || !sige_hip_upsample_phase_tile3_supported(C, Cout) || ((H | W) & 1)) return SIGE_HIP_EUNSUPPORTED;
    // (odd origins + odd offsets: a tile's output block starts on an even hi-res pixel.  The offsets can be checked here, the origins
    //  are the caller's precondition: include/sige_hip.h)
    if (!(offsetH & 1) || !(offsetW & 1)) return SIGE_HIP_EUNSUPPORTED;
    const long T = (long)B * N;
    if (T == 0) return SIGE_HIP_OK;
    const long blocks = (T + GP8::TPW - 1) / GP8::TPW * (Cout / 64) * 4;
    if (min_blocks <= 0 || blocks < min_blocks) return SIGE_HIP_EUNSUPPORTED;
    if (sige::g_plan_rec || conv_side_armed()) return SIGE_HIP_EUNSUPPORTED;
    if (!x || !active_indices || !packed_phase3 || !out) return SIGE_HIP_EINVAL;
    if (int rc = out_affine_status(out_scale, out_shift)) return rc;
    if (out_scale && !act_known(out_activation)) return SIGE_HIP_EUNSUPPORTED;
    const TwinOut twins[2] = {{twin0, twin0_scale, twin0_shift}, {twin1, twin1_scale, twin1_shift}};
    if (int rc = twins_status(twins)) return rc;
    // 32-bit byte offsets in the kernel: the source, and the grid's x extent
    if (!offsets_fit((long)B * (H / 2) * (W / 2) * C) || blocks / 4 > 0x7fffffffL || T > 0x7fffffffL) return SIGE_HIP_EUNSUPPORTED;
    if (!aligned16({x, packed_phase3, out, bias, residual, out_scale, out_shift}) || !twins_aligned(twins)) return SIGE_HIP_EUNSUPPORTED;
    Tile3Args a{};
    if (edit_shift_status(H, B, &a.hp_shift) != SIGE_HIP_OK) return SIGE_HIP_EUNSUPPORTED;
    hipStream_t st = as_stream(stream);
    if (int rc = flush_for_phase_tile3(x, residual, out, twin0, twin1, st)) return rc;
    a.x = x; a.x2 = x; a.idx = active_indices; a.packed = packed_phase3; a.bias = bias; a.residual = residual;
    a.oscale = out_scale; a.oshift = out_shift; a.oact = out_activation; a.out = out;
    a.twin0 = twin0; a.tscale0 = twin0_scale; a.tshift0 = twin0_shift;
    a.twin1 = twin1; a.tscale1 = twin1_scale; a.tshift1 = twin1_shift;
    a.B = B; a.N = N; a.T = (int)T; a.H = H; a.W = W; a.C1 = C; a.Cout = Cout; a.up = 1;
    a.Ho = Ho; a.Wo = Wo; a.offH = offsetH; a.offW = offsetW;
    a.ntn = Cout / 64; a.nchunks = a.nchunks1 = C / 64;
    if (compute == 1) launch_conv_tile3_phase<8, WIDE_F16>(a, st);
    else launch_conv_tile3_phase<8, WIDE_F32>(a, st);
    return launch_status(1);
}
