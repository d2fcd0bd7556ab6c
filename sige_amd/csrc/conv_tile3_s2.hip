// conv_tile3.hpp instantiated over the 5x5 windows of a 3x3 / stride-2 conv (Tile3GeoS2): eight tiles x 64 output
// channels per workgroup, fp16 operands only (exact fp32 and f16x3 stay on conv_mfma.hpp's ConvGeo<3, 2, 5, *>); the weight pack in
// the v3 stream order, and the C ABI.  Resources of the instance (code-object metadata, gfx950): DESIGN.md 5.31.
#include "conv_call.hpp"
#include "conv_tile3.hpp"

namespace sige {

using GS8H = Tile3GeoS2<8, WIDE_F16>;

bool conv_side_armed();  // (block_conv.hip)
int flush_for_phase_tile3(const float *x, const float *residual, float *out, float *twin0, float *twin1, hipStream_t st);

// packed[ntile][wave][chunk][tap = 3 kh + kw][nt][lane = (kq, j)][e]: the stream sige_hip_wide_conv_pack(prec = 0) lays out for the
// 9-tap fp16 tile conv v3 -- e < 8, channel ci = 64 chunk + 16 wave + 8 kq + e, rounded RNE and saturated -- and behind it
// kWidePadSteps steps of zeros, written here too (`halves` = the stream, `total` = stream + padding)
__global__ void pack_down3_f16_kernel(const float *__restrict__ w, int Cout, int Cin, _Float16 *__restrict__ packed, unsigned halves, unsigned total) {
    const unsigned nchunks = Cin / GS8H::CC;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {  // (32-bit: the host checks)
        if (i >= halves) {
            packed[i] = (_Float16)0.0f;
            continue;
        }
        unsigned r = i;
        const int e = r % 8; r /= 8;
        const int j = r % 32; r /= 32;
        const int kq = r % 2; r /= 2;
        const int nt = r % 2; r /= 2;
        const int tap = r % GS8H::KK; r /= GS8H::KK;
        const int chunk = r % nchunks; r /= nchunks;
        const int wave = r % 4; r /= 4;
        const int ntile = (int)r;
        const int co = 64 * ntile + 32 * nt + j;
        const int ci = chunk * GS8H::CC + wave * GS8H::CW + 8 * kq + e;
        const float v = w[((size_t)co * Cin + ci) * GS8H::KK + tap];
        packed[i] = (_Float16)fminf(fmaxf(v, -65504.0f), 65504.0f);
    }
}

static long down3_stream_bytes(int Cout, int Cin) { return (long)(Cout / 64) * 4 * (Cin / 64) * GS8H::STEPS * GS8H::STEPB; }

}  // namespace sige

using namespace sige;

extern "C" int sige_hip_down_tile3_supported(int C, int Cout) {
    return (C > 0 && C % 64 == 0 && Cout > 0 && Cout % 64 == 0) ? 1 : 0;
}

extern "C" size_t sige_hip_down_tile3_packed_size(int Cout, int Cin) {
    if (!sige_hip_down_tile3_supported(Cin, Cout)) return 0;
    return (size_t)((down3_stream_bytes(Cout, Cin) + (long)kWidePadSteps * GS8H::STEPB) / 4);
}

extern "C" int sige_hip_down_tile3_pack(const float *w, int Cout, int Cin, float *packed, void *stream) {
    if (!w || !packed) return SIGE_HIP_EINVAL;
    if (!sige_hip_down_tile3_supported(Cin, Cout)) return SIGE_HIP_EUNSUPPORTED;
    const long halves = down3_stream_bytes(Cout, Cin) / 2, total = halves + (long)kWidePadSteps * GS8H::STEPB / 2;
    if (total >= (1L << 31)) return SIGE_HIP_EUNSUPPORTED;  // (32-bit indices in the pack kernel: beyond 15 000 x 15 000 channels)
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    pack_down3_f16_kernel<<<grid, 256, 0, as_stream(stream)>>>(w, Cout, Cin, reinterpret_cast<_Float16 *>(packed), (unsigned)halves, (unsigned)total);
    return launch_status(1);
}

// This entry point has no launch-plan hook (as sige_hip_upsample_phase_tile3_nhwc): while a plan records it refuses, and the plan
// records the call the binding makes next.
extern "C" int sige_hip_down_tile3_nhwc(
        int compute, const float *x, int B, int C, int H, int W, const int32_t *active_indices, int N,
        const float *packed_down3, const float *bias, int Cout, int offsetH, int offsetW, const float *residual, int Ho, int Wo,
        const float *out_scale, const float *out_shift, int out_activation,
        float *twin0, const float *twin0_scale, const float *twin0_shift,
        float *twin1, const float *twin1_scale, const float *twin1_shift,
        int min_blocks, float *out, void *stream) {
    if (compute < 0 || compute > 2) return SIGE_HIP_EINVAL;
    if (B < 0 || N < 0 || C <= 0 || Cout <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return SIGE_HIP_EINVAL;
    if (compute != 1 || !sige_hip_down_tile3_supported(C, Cout)) return SIGE_HIP_EUNSUPPORTED;
    const long T = (long)B * N;
    if (T == 0) return SIGE_HIP_OK;
    const long blocks = (T + GS8H::TPW - 1) / GS8H::TPW * (Cout / 64);
    if (min_blocks <= 0 || blocks < min_blocks) return SIGE_HIP_EUNSUPPORTED;
    if (sige::g_plan_rec || conv_side_armed()) return SIGE_HIP_EUNSUPPORTED;
    if (!x || !active_indices || !packed_down3 || !out) return SIGE_HIP_EINVAL;
    if (int rc = out_affine_status(out_scale, out_shift)) return rc;
    if (out_scale && !act_known(out_activation)) return SIGE_HIP_EUNSUPPORTED;
    const TwinOut twins[2] = {{twin0, twin0_scale, twin0_shift}, {twin1, twin1_scale, twin1_shift}};
    if (int rc = twins_status(twins)) return rc;
    // 32-bit byte offsets in the kernel: the source, and the grid's x extent
    if (!offsets_fit((long)B * H * W * C) || blocks > 0x7fffffffL || T > 0x7fffffffL) return SIGE_HIP_EUNSUPPORTED;
    if (!aligned16({x, packed_down3, out, bias, residual, out_scale, out_shift}) || !twins_aligned(twins)) return SIGE_HIP_EUNSUPPORTED;
    Tile3Args a{};
    if (edit_shift_status(H, B, &a.hp_shift) != SIGE_HIP_OK) return SIGE_HIP_EUNSUPPORTED;
    hipStream_t st = as_stream(stream);
    if (int rc = flush_for_phase_tile3(x, residual, out, twin0, twin1, st)) return rc;
    a.x = x; a.x2 = x; a.idx = active_indices; a.packed = packed_down3; a.bias = bias; a.residual = residual;
    a.oscale = out_scale; a.oshift = out_shift; a.oact = out_activation; a.out = out;
    a.twin0 = twin0; a.tscale0 = twin0_scale; a.tshift0 = twin0_shift;
    a.twin1 = twin1; a.tscale1 = twin1_scale; a.tshift1 = twin1_shift;
    a.B = B; a.N = N; a.T = (int)T; a.H = H; a.W = W; a.C1 = C; a.Cout = Cout;
    a.Ho = Ho; a.Wo = Wo; a.offH = offsetH; a.offW = offsetW;
    a.ntn = Cout / 64; a.nchunks = a.nchunks1 = C / 64;
    conv_tile3_kernel<GS8H, T3_GATHER, false, false, true><<<(unsigned)blocks, 256, 0, st>>>(a);
    return launch_status(1);
}
