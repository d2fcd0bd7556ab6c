// Latent head of Stable Diffusion's VAE encoder: norm_out -> SiLU -> conv_out (3x3 / padding 1, C <= 512 -> 2 z = 8 channels) with
// the autoencoder's 1x1 quant_conv folded into the weights and, optionally, the posterior sample behind it
// (sige_model.py:272-275, ldm/models/autoencoder.py encode(), distributions.py DiagonalGaussianDistribution.sample).
//
// norm_out is a true GroupNorm of the edited activation, so the reference runs this tail densely in every mode: at a small edit it
// is a fixed cost the tiles do not shrink.  conv_out.hip's kernels stop at 4 output channels, and its matrix-core form keeps C / 2
// weights per lane in registers, which cannot hold at C = 512 with 72 tap columns.  Here the same tap-as-columns GEMM
//     P[p][tap*Cout + co] = sum_ch act(scale[ch] * x[p][ch] + shift[ch]) * w[co][ch][tap]    M = pixels, N = 9 Cout, K = C
// runs on v_mfma_f32_16x16x4_f32 (exact fp32 operands) with the weights STREAMED through LDS in chunks of 64 channels:
//   * one workgroup = a 6x6 output tile: its (6+2)^2 = 64 halo pixels are four M-blocks of 16, one per wave;
//   * lane (kq, r) of a wave owns pixel r of the block and channels 16 t + 4 kq .. + 3 (t = 0..3) of a chunk: four 16-byte loads,
//     issued one chunk ahead of their use together with the thread's share of the next chunk's weights;
//   * B fragments come from the chunk's [64 channels][9 Cout columns] LDS image (pitch = 4 mod 8 floats: the two k rows a
//     32-lane group reads lie 16 banks apart);
//   * P replaces the weights in LDS, and the 9-term shifted sum out[y][x][co] = sum_tap P[(y+dy, x+dx)][tap*Cout + co] follows;
//     out-of-image taps are skipped by the summing lane: that is the zero padding of the ACTIVATED tensor.
// The real shape is 64x64 pixels = 121 tiles on 256 CUs, so the channels are split over up to 8 workgroups per tile
// (blocks <= 512): each writes its 36 Cout partial sums to a workspace slice with device-coherent stores and draws a ticket; the
// last one to arrive adds the slices IN SPLIT ORDER, its own included -- the in-launch split finish of
// split_finish.hpp, one launch, no float atomics, bit-identical from run to run.
#include <algorithm>

#include "split_finish.hpp"

namespace sige {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kLT = 6, kLP = kLT + 2, kLPix = kLP * kLP;  // output tile edge, halo edge, halo pixels (= 4 M-blocks of 16)
constexpr int kLKC = 64;                                    // channels per weight chunk
constexpr int kLMaxC = 512, kLMaxSplit = 8, kLMaxCout = 16;
// workgroups the channel split aims at: two per CU, so that one's start-up and finish overlap the other's matrix work (measured at
// [1,512,64,64] -> 8, 121 tiles: 26.7 us unsplit, 18.0 us at <= 256 workgroups, 17.3 us at <= 512, 24.7 us at <= 1024)
constexpr long kLTargetBlocks = 512;
static_assert(kLPix == 64, "one 16-pixel M-block per wave");

struct LatentHeadArgs {
    const float *x, *scale, *shift, *w, *bias, *noise;
    float *out, *z, *ws;
    int32_t *tickets;
    int B, C, H, W, Cout, aff_sb, act, tilesW, ksplit, cps, nchunks;
    float latent_scale;
};
static_assert(sizeof(LatentHeadArgs) >= 128, "kernarg_touch<128>");

// NB = 16-wide column blocks of the GEMM: ceil(9 Cout / 16)
template <int NB>
__global__ __launch_bounds__(256) void conv_latent_head_kernel(LatentHeadArgs a) {
    kernarg_touch<128>();
    constexpr int PITCH = 16 * NB + 4;
    constexpr int WV = (144 * ((16 * NB) / 9) + 255) / 256;  // 16-byte weight loads per thread and chunk at the largest Cout of this NB
    constexpr int NO = (kLT * kLT * kLMaxCout + 255) / 256;  // outputs per thread
    __shared__ __attribute__((aligned(16))) float L[kLKC * PITCH];  // the chunk's weights [channel][column]; then P [halo pixel][column]
    __shared__ __attribute__((aligned(16))) float s_sc[kLMaxC], s_sh[kLMaxC];
    __shared__ float fin[kLT * kLT * kLMaxCout];
    __shared__ int ticket_lds;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const int split = blockIdx.x, tile = blockIdx.y, b = blockIdx.z;
    const int C = a.C, H = a.H, W = a.W, Cout = a.Cout;
    const int h0 = (tile / a.tilesW) * kLT, w0 = (tile % a.tilesW) * kLT;
    const int ch0 = split * a.cps, ch1 = min(ch0 + a.cps, a.nchunks);

    // this lane's pixel (clamped: a halo pixel outside the image reads a valid address; nobody sums it)
    const float *xp;
    {
        const int p = 16 * wave + j;
        const int h = min(max(h0 + (p >> 3) - 1, 0), H - 1), ww = min(max(w0 + (p & 7) - 1, 0), W - 1);
        xp = a.x + (((size_t)b * H + h) * W + ww) * C + 4 * kq;
    }
    float4 raw[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) raw[t] = *reinterpret_cast<const float4 *>(xp + ch0 * kLKC + 16 * t);

    // the thread's share of a chunk's weights: w[co][c0 .. c0+63][tap] is 576 contiguous floats per output channel
    const int E4 = 144 * Cout;
    float4 wreg[WV];
    auto load_weights = [&](int chunk) {
#pragma unroll
        for (int n = 0; n < WV; ++n) {
            const int i = 4 * min(tid + 256 * n, E4 - 1);  // (past the end: the last unit again, not stored)
            const int co = i / 576, rem = i % 576;
            wreg[n] = *reinterpret_cast<const float4 *>(a.w + ((size_t)co * C + chunk * kLKC) * 9 + rem);
        }
    };
    auto store_weights = [&]() {
#pragma unroll
        for (int n = 0; n < WV; ++n) {
            const int i4 = tid + 256 * n;
            if (i4 < E4) {
                const int i = 4 * i4;
                const int co = i / 576, rem = i % 576;
                const float v[4] = {wreg[n].x, wreg[n].y, wreg[n].z, wreg[n].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) L[((rem + e) / 9) * PITCH + ((rem + e) % 9) * Cout + co] = v[e];
            }
        }
    };
    load_weights(ch0);

    // columns >= 9 Cout are never staged: zero once (their products are never summed)
    for (int i = tid; i < kLKC * PITCH; i += 256) L[i] = 0.f;
    {
        const int n = (ch1 - ch0) * kLKC;
#pragma unroll
        for (int it = 0; it < kLMaxC / 256; ++it) {
            const int c = tid + 256 * it, cc = ch0 * kLKC + min(c, n - 1);
            const float s = a.scale ? a.scale[b * a.aff_sb + cc] : 1.f;
            const float t = a.shift ? a.shift[b * a.aff_sb + cc] : 0.f;
            if (c < n) { s_sc[c] = s; s_sh[c] = t; }
        }
    }
    __syncthreads();
    store_weights();
    __syncthreads();

    floatx4 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = floatx4{0.f, 0.f, 0.f, 0.f};

    for (int ch = ch0; ch < ch1; ++ch) {
        float av[16];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = (ch - ch0) * kLKC + 16 * t + 4 * kq;
            const float4 s4 = *reinterpret_cast<const float4 *>(s_sc + c);
            const float4 t4 = *reinterpret_cast<const float4 *>(s_sh + c);
            float4 v = raw[t];
            v.x = s4.x * v.x; v.y = s4.y * v.y; v.z = s4.z * v.z; v.w = s4.w * v.w;
            v.x = t4.x + v.x; v.y = t4.y + v.y; v.z = t4.z + v.z; v.w = t4.w + v.w;
            if (a.act == SIGE_HIP_ACT_SWISH) { v.x = swish(v.x); v.y = swish(v.y); v.z = swish(v.z); v.w = swish(v.w); }  // (uniform)
            av[4 * t] = v.x; av[4 * t + 1] = v.y; av[4 * t + 2] = v.z; av[4 * t + 3] = v.w;
        }
        if (ch + 1 < ch1) {  // (workgroup-uniform) the next chunk's pixels and weights while this one is in the matrix pipe
#pragma unroll
            for (int t = 0; t < 4; ++t) raw[t] = *reinterpret_cast<const float4 *>(xp + (ch + 1) * kLKC + 16 * t);
            load_weights(ch + 1);
        }
        // k-step s = 4 t + e: channel 16 t + 4 kq + e of the chunk on both operands.  The B values of four k-steps are read as one
        // batch, a batch ahead of the MFMAs that use them; the scheduling barriers keep the batches whole (left alone, the
        // compiler sank every read to its use: read, wait for the LDS round trip, two MFMAs -- the matrix pipe idle most of the time)
        float bb[2][4][NB];
        auto read_b = [&](int t, float (&dst)[4][NB]) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float *brow = L + (16 * t + 4 * kq + e) * PITCH + j;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) dst[e][nb] = brow[16 * nb];
            }
        };
        read_b(0, bb[0]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t + 1 < 4) read_b(t + 1, bb[(t + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[4 * t + e], bb[t & 1][e][nb], acc[nb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        if (ch + 1 < ch1) store_weights();
        __syncthreads();
    }

    // P: reg r of lane (kq, j) = halo pixel 16 wave + 4 kq + r, column 16 nb + j
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) L[(16 * wave + 4 * kq + r) * PITCH + 16 * nb + j] = acc[nb][r];
    }
    __syncthreads();

    // the shifted sum: thread -> (output pixel, channel) idx = tid + 256 n
    const int NOUT = kLT * kLT * Cout;
    float val[NO];
#pragma unroll
    for (int n = 0; n < NO; ++n) {
        const int idx = min(tid + 256 * n, NOUT - 1);
        const int op = idx / Cout, co = idx - op * Cout;
        const int oy = op / kLT, ox = op - oy * kLT;
        float v[9];  // (the nine reads as one batch: summed as they were written, each waited for its own LDS round trip)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) v[tap] = L[((oy + tap / 3) * kLP + ox + tap % 3) * PITCH + tap * Cout + co];
        __builtin_amdgcn_sched_barrier(0);
        float s = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ih = h0 + oy + tap / 3 - 1, iw = w0 + ox + tap % 3 - 1;
            s += (ih >= 0 && ih < H && iw >= 0 && iw < W) ? v[tap] : 0.f;
        }
        val[n] = s;
    }

    if (a.ksplit > 1) {
        // ---- channel split: this workgroup's sums to its workspace slice, a ticket, the last split of the tile adds them up ----
        const int unit = b * gridDim.y + tile;
        float *const ws = a.ws + (size_t)unit * a.ksplit * NOUT;
#pragma unroll
        for (int n = 0; n < NO; ++n) {
            const int idx = tid + 256 * n;
            if (idx < NOUT) coherent_store(ws + (size_t)split * NOUT + idx, val[n]);
        }
        if (!split_arrive_last(a.tickets + unit, a.ksplit, &ticket_lds)) return;  // (the protocol: split_finish.hpp)
#pragma unroll
        for (int n = 0; n < NO; ++n) {
            const int idx = min(tid + 256 * n, NOUT - 1);
            float part[kLMaxSplit];
#pragma unroll
            for (int u = 0; u < kLMaxSplit; ++u)  // (past the end: the last slice again, not used)
                part[u] = coherent_load(ws + (size_t)min(u, a.ksplit - 1) * NOUT + idx);
            float s = 0.f;
#pragma unroll
            for (int u = 0; u < kLMaxSplit; ++u) s += u < a.ksplit ? part[u] : 0.f;
            val[n] = s;
        }
    }

    // bias, the moments, and their image in LDS for the posterior
#pragma unroll
    for (int n = 0; n < NO; ++n) {
        const int idx = tid + 256 * n, ci = min(idx, NOUT - 1);
        const int op = ci / Cout, co = ci - op * Cout;
        const int oy = op / kLT, ox = op - oy * kLT;
        const int h = h0 + oy, ww = w0 + ox;
        const float v = (a.bias ? a.bias[co] : 0.f) + val[n];
        if (idx < NOUT) {
            fin[idx] = v;
            if (h < H && ww < W) a.out[(((size_t)b * H + h) * W + ww) * Cout + co] = v;
        }
    }
    if (!a.z) return;  // (uniform)
    __syncthreads();
    // z = latent_scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise): mean = channels [0, Cout/2), logvar the rest
    const int Z = Cout >> 1, NZ = kLT * kLT * Z;
#pragma unroll
    for (int n = 0; n < (NO + 1) / 2; ++n) {
        const int idx = tid + 256 * n, ci = min(idx, NZ - 1);
        const int op = ci / Z, zc = ci - op * Z;
        const int oy = op / kLT, ox = op - oy * kLT;
        const int h = h0 + oy, ww = w0 + ox;
        const size_t pix = ((size_t)b * H + min(h, H - 1)) * W + min(ww, W - 1);  // (clamped: the load is not behind the bounds test)
        const float eps = a.noise ? a.noise[pix * Z + zc] : 0.f;
        const float mean = fin[op * Cout + zc];
        const float lv = fminf(fmaxf(fin[op * Cout + Z + zc], -30.0f), 20.0f);
        const float v = a.latent_scale * (mean + expf(0.5f * lv) * eps);
        if (idx < NZ && h < H && ww < W) a.z[pix * Z + zc] = v;
    }
}

}  // namespace sige

using namespace sige;

extern "C" int sige_hip_conv3x3_latent_head_nhwc_f32(const float *x, int B, int C, int H, int W,
                                                     const float *scale, int scaleB, int scaleC,
                                                     const float *shift, int shiftB, int shiftC, int activation,
                                                     const float *weight, const float *bias, int Cout, float *out,
                                                     const float *noise, float latent_scale, float *z, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_conv3x3_latent_head_nhwc_f32, x, B, C, H, W, scale, scaleB, scaleC, shift, shiftB, shiftC, activation, weight,
                   bias, Cout, out, noise, latent_scale, z, stream);
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || Cout <= 0) return SIGE_HIP_EINVAL;
    if (!x || !weight || !out || (noise && !z)) return SIGE_HIP_EINVAL;
    if (activation != SIGE_HIP_ACT_IDENTITY && activation != SIGE_HIP_ACT_SWISH) return SIGE_HIP_EUNSUPPORTED;
    if (Cout < 5 || Cout > kLMaxCout || C % kLKC || C > kLMaxC) return SIGE_HIP_EUNSUPPORTED;
    if (z && (Cout & 1)) return SIGE_HIP_EUNSUPPORTED;
    if ((scale == nullptr) != (shift == nullptr)) return SIGE_HIP_EUNSUPPORTED;
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!al(x) || !al(weight) || !al(bias) || !al(out) || !al(noise) || !al(z)) return SIGE_HIP_EUNSUPPORTED;
    int aff_sb = 0;
    if (scale) {
        if (scaleC != C || shiftC != C || scaleB != shiftB || !(scaleB == 1 || scaleB == B)) return SIGE_HIP_EUNSUPPORTED;
        if (!al(scale) || !al(shift)) return SIGE_HIP_EUNSUPPORTED;
        aff_sb = scaleB > 1 ? C : 0;
    }
    const int tilesH = ceil_div(H, kLT), tilesW = ceil_div(W, kLT);
    const long tiles = (long)tilesH * tilesW, units = tiles * B;
    if (tiles > 65535 || B > 65535 || units > 0x7fffffffL / (kLT * kLT * kLMaxCout * kLMaxSplit)) return SIGE_HIP_EUNSUPPORTED;  // (grid y / z)
    hipStream_t st = as_stream(stream);

    // channel split: at most two workgroups per CU in all, whole chunks, at most 8 slices to add up
    LatentHeadArgs a;
    a.nchunks = C / kLKC;
    a.ws = nullptr; a.tickets = nullptr;
    int ksplit = (int)std::min<long>(std::min<long>(kLTargetBlocks / units, a.nchunks), kLMaxSplit);
    if (ksplit > 1) {
        a.tickets = split_tickets(st, units);
        if (a.tickets) a.ws = split_workspace(st, (size_t)units * ksplit * kLT * kLT * Cout);
        if (!a.tickets || !a.ws) ksplit = 1;
    }
    if (ksplit < 1) ksplit = 1;
    a.cps = ceil_div(a.nchunks, ksplit);
    a.ksplit = ceil_div(a.nchunks, a.cps);  // (no empty split)
    a.x = x; a.scale = scale; a.shift = shift; a.w = weight; a.bias = bias; a.noise = noise;
    a.out = out; a.z = z;
    a.B = B; a.C = C; a.H = H; a.W = W; a.Cout = Cout; a.aff_sb = aff_sb; a.act = activation; a.tilesW = tilesW;
    a.latent_scale = latent_scale;
    const dim3 grid((unsigned)a.ksplit, (unsigned)tiles, (unsigned)B);
    switch ((9 * Cout + 15) / 16) {
        case 3: conv_latent_head_kernel<3><<<grid, 256, 0, st>>>(a); break;
        case 4: conv_latent_head_kernel<4><<<grid, 256, 0, st>>>(a); break;
        case 5: conv_latent_head_kernel<5><<<grid, 256, 0, st>>>(a); break;
        case 6: conv_latent_head_kernel<6><<<grid, 256, 0, st>>>(a); break;
        case 7: conv_latent_head_kernel<7><<<grid, 256, 0, st>>>(a); break;
        case 8: conv_latent_head_kernel<8><<<grid, 256, 0, st>>>(a); break;
        case 9: conv_latent_head_kernel<9><<<grid, 256, 0, st>>>(a); break;
        default: return SIGE_HIP_EUNSUPPORTED;
    }
    return launch_status();
}
