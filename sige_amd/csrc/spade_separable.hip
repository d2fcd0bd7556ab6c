// gamma | beta of a GAN-Compression ("sub-mobile") SPADE layer in ONE launch: two separable convs of the label features
// (gaugan/models/mobile_modules.py:65-119 SIGESeparableConv2d, used by sige_normalization.py:91-170 SIGEFusedSubMobileSPADE):
//     d_b[p][c]          = sum_tap dw_b[c][tap] * a[p + tap][c] + dwb_b[c]          depthwise 3x3 / padding 1           (VALU)
//     n_b[p][c]          = s_b[c] * d_b[p][c] + t_b[c]                               the InstanceNorm as its cached affine (VALU)
//     gb[p][b * oc + o]  = sum_c pw_b[o][c] * n_b[p][c] + pwb_b[o]                   pointwise 1x1, b in {gamma, beta}   (MFMA)
// The affine between the two convs changes with every original image, so the pair cannot be folded into one packed 3x3 weight;
// as modules it is a scalar grouped tile conv, a torch affine and a 1x1 tile conv per branch and a torch.cat behind them.
//
// Two source forms with the same arithmetic in the same order:
//   tiled: a = tile slab [T][6][6][Ch] with its halo (one part of what scatter_gather_split writes), gb = [T][4][4][2 oc];
//   dense: a = [H][W][Ch] with zero padding at the image border, gb = [H][W][2 oc]; pixels are taken 16 at a time in row-major order.
// Either way 16 output pixels are one "pixel block" and output pixel q of the launch is row q of gb.
//
// Decomposition.  A workgroup (4 waves) owns MB pixel blocks x CB column blocks of 16 output channels of ONE branch, MB * CB = 4,
// chosen by oc (CB = 4 | 2 | 1 for >= 4 | 2-3 | 1 column blocks): no wave idles at oc = 8.
//   1. all threads: n_b of the workgroup's 16 MB pixels -> LDS, one (pixel, channel quad) per thread and step: 9 + 9 + 3 16-byte
//      loads, 144 multiplies and adds.  Workgroups of other column groups recompute it: cheap next to a second launch.
//   2. wave (mb, cb): v_mfma_f32_16x16x4_f32 (exact fp32 products, k-ordered fp32 sums) with the WEIGHTS as the row operand,
//      D[o][p] = sum_c pw[o][c] n[p][c]: lane (kq, j) ends with output channels o0 + 4 kq .. + 3 of pixel j -- one 16-byte store.
//      Lane (kq, j) feeds channel 16 t + 4 kq + e at k-step 4 t + e on both operands: one 16-byte weight load from global memory
//      (issued before step 1) and one 16-byte LDS read per 16 channels.  Two accumulators (e even / odd) keep the matrix pipe fed.
// A column block lies inside one branch (the branch is blockIdx.z); a ragged last block and the channels between Ch and the next
// multiple of 16 are masked by value: every load has a clamped, valid address and none sits behind a lane-dependent branch.
// No atomics, no workspace: bit-identical from run to run.
//
// Stacked edits (sige_hip_set_edit_batch): the dense form over E images of h = 2^s rows each, [E h][W][Ch] (..._images_nhwc_f32).
// Pixel (y, x) belongs to image e = y >> s: its taps are zero outside rows [e h, (e + 1) h) and its affine is row e of [E][2][Ch].
// Only the tap mask and the affine's address change; E = 1 is s = 0 with affine stride 0 and is the plain dense form bit for bit.
//
// The affine of a DENSE layer is the InstanceNorm of d_b over ONE image, recomputed for every edit (mobile_modules.py:116):
// spade_separable_stats_kernel, one workgroup per (16-channel group, branch, image), 4 channel quads x 64 pixel slots.  Two passes
// inside the launch, d_b recomputed in the tap order of step 1: mean_b[c] first, then sum (d - mean)^2 -- E[d^2] - E[d]^2 loses
// the variance to cancellation once |mean| / sigma reaches 100.  A slot adds its pixels p = slot, slot + 64, ... in that order, the 64
// slots of a channel are added through LDS as 4 x 16 in slot order, then 4: the order depends on (h, W) alone, so image e of a
// stacked call has the bits of a single-image call on it.
#include "common.hpp"

namespace sige {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kSepMinCh = 8, kSepMaxCh = 128, kSepMinOc = 4, kSepMaxOc = 1024;
constexpr int kSepMaxPix = 64;  // pixels of a workgroup at MB = 4

struct SepArgs {
    const float *a, *dw_w, *dw_b, *sc, *sh, *pw_w, *pw_b;
    float *out;
    long npb;          // pixel blocks of the launch
    int H, W, Ch, oc;  // (tiled: H = W = 6)
    int mb_shift;      // MB = 1 << mb_shift pixel blocks per workgroup; CB = 4 >> mb_shift column blocks
    int img_shift;     // dense: log2 of the rows of ONE image when several are stacked along H; 0 = one image of H rows
    int aff_stride;    // dense: floats from one image's sc / sh to the next one's (0 = one affine for every row)
    int pad;
};
static_assert(sizeof(SepArgs) >= 96, "kernarg_touch<96>");

__device__ __forceinline__ float4 sel4(bool keep, float4 v) { return keep ? v : make_float4(0.f, 0.f, 0.f, 0.f); }

// KT = ceil(Ch / 16): 16-channel steps of the GEMM
template <int KT, bool TILED>
__global__ __launch_bounds__(256) void spade_separable_kernel(SepArgs g) {
    kernarg_touch<96>();
    constexpr int QP = 4 * KT;        // channel quads incl. the padding up to 16 KT
    constexpr int PITCH = 16 * KT + 4;
    __shared__ __attribute__((aligned(16))) float Ln[kSepMaxPix * PITCH];  // n_b [local pixel][channel]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const int Ch = g.Ch, oc = g.oc, H = g.H, W = g.W, br = blockIdx.z;
    const int mb_shift = g.mb_shift, MB = 1 << mb_shift, CB = 4 >> mb_shift;
    const long npb = g.npb;
    const long npix = TILED ? npb * 16 : (long)H * W;  // output pixels of the launch

    // ---- this wave's GEMM operand: rows o0 + j of pw_b, issued now, used after step 1 ----
    const int mb = wave >> (2 - mb_shift), cb = wave & (CB - 1);
    const int o0 = 16 * ((int)blockIdx.y * CB + cb);
    float4 wa[KT];
    {
        const float *wrow = g.pw_w + ((size_t)br * oc + min(o0 + j, oc - 1)) * Ch;
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int c0 = 16 * t + 4 * kq;
            wa[t] = sel4(c0 < Ch && o0 + j < oc, *reinterpret_cast<const float4 *>(wrow + min(c0, Ch - 4)));
        }
    }
    const float4 pb = *reinterpret_cast<const float4 *>(g.pw_b + (size_t)br * oc + min(o0 + 4 * kq, oc - 4));

    // ---- step 1: n_b of 16 MB pixels x Ch channels ----
    const int items = 16 * MB * QP;
    for (int it = 0; it < items; it += 256) {  // (workgroup-uniform trip count: items is a multiple of 64 KT, clamped below)
        const int i = it + tid, ii = min(i, items - 1);
        const int pl = ii / QP, qd = ii - pl * QP;  // (QP is a compile-time constant)
        const int c0 = 4 * qd, cc = min(c0, Ch - 4);
        const long blk = (long)blockIdx.x * MB + (pl >> 4);
        const int p = pl & 15;
        float4 av[9];
        bool live;
        size_t aoff = 0;  // this pixel's affine within sc / sh (dense form over stacked images)
        if (TILED) {
            live = blk < npb;
            const float *base = g.a + (size_t)(blk < npb ? blk : npb - 1) * 36 * Ch + (size_t)((p >> 2) * 6 + (p & 3)) * Ch + cc;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) av[tap] = *reinterpret_cast<const float4 *>(base + ((tap / 3) * 6 + tap % 3) * Ch);
        } else {
            const long q = blk * 16 + p;
            live = q < npix;
            const unsigned qc = (unsigned)(q < npix ? q : npix - 1);  // (H * W < 2^31: checked by the entry point)
            const int y = (int)(qc / (unsigned)W), x = (int)(qc - (unsigned)y * (unsigned)W);
            // the rows of this pixel's image: [0, H), or [e h, (e + 1) h) of image e = y >> s when images are stacked
            const int s = g.img_shift, e = s ? y >> s : 0, y0 = e << s, y1 = s ? y0 + (1 << s) : H;
            aoff = (size_t)e * (size_t)g.aff_stride;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                const bool in = yy >= y0 && yy < y1 && xx >= 0 && xx < W;
                const float *ptr = g.a + ((size_t)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)) * Ch + cc;
                av[tap] = sel4(in, *reinterpret_cast<const float4 *>(ptr));  // (clamped address, zero padding by value)
            }
        }
        // the depthwise weights of the quad: dw_b[cc .. cc+3][0..8] are 36 contiguous floats
        float wf[36];
        {
            const float *wp = g.dw_w + ((size_t)br * Ch + cc) * 9;
#pragma unroll
            for (int n = 0; n < 9; ++n) {
                const float4 v = *reinterpret_cast<const float4 *>(wp + 4 * n);
                wf[4 * n] = v.x; wf[4 * n + 1] = v.y; wf[4 * n + 2] = v.z; wf[4 * n + 3] = v.w;
            }
        }
        const float4 b4 = *reinterpret_cast<const float4 *>(g.dw_b + (size_t)br * Ch + cc);
        const float4 s4 = *reinterpret_cast<const float4 *>(g.sc + aoff + (size_t)br * Ch + cc);
        const float4 t4 = *reinterpret_cast<const float4 *>(g.sh + aoff + (size_t)br * Ch + cc);
        float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float x4[4] = {av[tap].x, av[tap].y, av[tap].z, av[tap].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] += wf[9 * e + tap] * x4[e];
        }
        float4 n;
        n.x = t4.x + s4.x * (d[0] + b4.x);
        n.y = t4.y + s4.y * (d[1] + b4.y);
        n.z = t4.z + s4.z * (d[2] + b4.z);
        n.w = t4.w + s4.w * (d[3] + b4.w);
        if (i < items) *reinterpret_cast<float4 *>(Ln + pl * PITCH + c0) = sel4(live && c0 < Ch, n);
    }
    __syncthreads();

    // ---- step 2: this wave's 16 output channels x 16 pixels ----
    const long blk = (long)blockIdx.x * MB + mb;
    if (__builtin_amdgcn_readfirstlane((int)(o0 >= oc || blk >= npb))) return;  // (one value per wave: a scalar branch)
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float *nrow = Ln + (16 * mb + j) * PITCH + 4 * kq;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const float4 nb = *reinterpret_cast<const float4 *>(nrow + 16 * t);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t].x, nb.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t].y, nb.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t].z, nb.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t].w, nb.w, acc1, 0, 0, 0);
    }
    // reg r of lane (kq, j) = output channel o0 + 4 kq + r of pixel j
    const long q = blk * 16 + j;
    float4 v;
    v.x = pb.x + (acc0[0] + acc1[0]);
    v.y = pb.y + (acc0[1] + acc1[1]);
    v.z = pb.z + (acc0[2] + acc1[2]);
    v.w = pb.w + (acc0[3] + acc1[3]);
    if (q < npix && o0 + 4 * kq < oc) store_out4(g.out + (size_t)q * 2 * oc + (size_t)br * oc + o0 + 4 * kq, v);
}

template <bool TILED>
static int sep_launch(const SepArgs &a, dim3 grid, hipStream_t st) {
    switch ((a.Ch + 15) / 16) {
        case 1: spade_separable_kernel<1, TILED><<<grid, 256, 0, st>>>(a); break;
        case 2: spade_separable_kernel<2, TILED><<<grid, 256, 0, st>>>(a); break;
        case 3: spade_separable_kernel<3, TILED><<<grid, 256, 0, st>>>(a); break;
        case 4: spade_separable_kernel<4, TILED><<<grid, 256, 0, st>>>(a); break;
        case 5: spade_separable_kernel<5, TILED><<<grid, 256, 0, st>>>(a); break;
        case 6: spade_separable_kernel<6, TILED><<<grid, 256, 0, st>>>(a); break;
        case 7: spade_separable_kernel<7, TILED><<<grid, 256, 0, st>>>(a); break;
        case 8: spade_separable_kernel<8, TILED><<<grid, 256, 0, st>>>(a); break;
        default: return SIGE_HIP_EUNSUPPORTED;
    }
    return launch_status();
}

// ---- InstanceNorm statistics of the depthwise output, per (image, branch, channel) ---------------------------------------------
struct SepStatsArgs {
    const float *a, *dw_w, *dw_b;
    float *out_sc, *out_sh;
    int h, W, Ch;  // ONE image: h rows; image e starts at row e h (blockIdx.z = e)
    float eps;
};
static_assert(sizeof(SepStatsArgs) >= 56, "kernarg_touch<56>");

constexpr int kStatSlots = 64;                 // pixel slots of a workgroup
constexpr int kStatPitch = 16 * 16 + 16;       // floats between the 16-slot parts in LDS: part k starts at bank 16 k

// sum over the 64 slots of this thread's channel quad, the same bits in every thread of the quad: 4 parts of 16 slots in slot
// order, then the 4 parts in order.  `L` [4 parts][16 slots][16 channels], `P` [4 parts][16 channels].
__device__ __forceinline__ float4 stat_sum(float4 v, float *L, float *P, int tid) {
    const int slot = tid >> 2, qd = tid & 3;
    *reinterpret_cast<float4 *>(L + (slot >> 4) * kStatPitch + (slot & 15) * 16 + 4 * qd) = v;
    __syncthreads();
    if (tid < 64) {  // (wave 0, whole: a scalar branch)
        const int c = tid & 15, part = tid >> 4;
        const float *src = L + part * kStatPitch + c;
        float acc = src[0];
#pragma unroll
        for (int k = 1; k < 16; ++k) acc += src[16 * k];
        P[16 * part + c] = acc;
    }
    __syncthreads();
    float4 r = *reinterpret_cast<const float4 *>(P + 4 * qd);
#pragma unroll
    for (int part = 1; part < 4; ++part) {
        const float4 q = *reinterpret_cast<const float4 *>(P + 16 * part + 4 * qd);
        r.x += q.x; r.y += q.y; r.z += q.z; r.w += q.w;
    }
    return r;
}

__global__ __launch_bounds__(256) void spade_separable_stats_kernel(SepStatsArgs g) {
    kernarg_touch<56>();
    __shared__ __attribute__((aligned(16))) float L[2][4 * kStatPitch];  // (one buffer per pass: no barrier between the passes)
    __shared__ __attribute__((aligned(16))) float P[2][64];

    const int tid = threadIdx.x, slot = tid >> 2, qd = tid & 3;
    const int h = g.h, W = g.W, Ch = g.Ch, br = blockIdx.y, img = blockIdx.z;
    const int c0 = 16 * (int)blockIdx.x + 4 * qd, cc = min(c0, Ch - 4);
    const unsigned n = (unsigned)h * (unsigned)W;  // pixels of one image (< 2^30: checked by the entry point)
    const float *a = g.a + (size_t)img * n * Ch + cc;

    // the depthwise weights of the quad: dw_b[cc .. cc+3][0..8] are 36 contiguous floats
    float wf[36];
    {
        const float *wp = g.dw_w + ((size_t)br * Ch + cc) * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float4 v = *reinterpret_cast<const float4 *>(wp + 4 * k);
            wf[4 * k] = v.x; wf[4 * k + 1] = v.y; wf[4 * k + 2] = v.z; wf[4 * k + 3] = v.w;
        }
    }
    const float4 b4 = *reinterpret_cast<const float4 *>(g.dw_b + (size_t)br * Ch + cc);

    // d_b + bias of pixel p of the image for the quad, in the tap order of spade_separable_kernel's step 1
    auto depthwise = [&](unsigned p, float (&d)[4]) {
        const int y = (int)(p / (unsigned)W), x = (int)(p - (unsigned)y * (unsigned)W);
        float4 av[9];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            const bool in = yy >= 0 && yy < h && xx >= 0 && xx < W;  // (the image's own border: a seam row is padding)
            const float *ptr = a + ((size_t)min(max(yy, 0), h - 1) * W + min(max(xx, 0), W - 1)) * Ch;
            av[tap] = sel4(in, *reinterpret_cast<const float4 *>(ptr));  // (clamped address, zero padding by value)
        }
        d[0] = d[1] = d[2] = d[3] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float x4[4] = {av[tap].x, av[tap].y, av[tap].z, av[tap].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] += wf[9 * e + tap] * x4[e];
        }
        d[0] += b4.x; d[1] += b4.y; d[2] += b4.z; d[3] += b4.w;
    };

    const float inv_n = 1.0f / (float)n;
    // ---- pass 1: the mean ----
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (unsigned p0 = 0; p0 < n; p0 += kStatSlots) {  // (workgroup-uniform trip count; the pixel is clamped, its value masked)
        const unsigned p = p0 + slot;
        float d[4];
        depthwise(min(p, n - 1), d);
        const bool live = p < n;
        acc.x += live ? d[0] : 0.f; acc.y += live ? d[1] : 0.f; acc.z += live ? d[2] : 0.f; acc.w += live ? d[3] : 0.f;
    }
    float4 mean = stat_sum(acc, L[0], P[0], tid);
    mean.x *= inv_n; mean.y *= inv_n; mean.z *= inv_n; mean.w *= inv_n;

    // ---- pass 2: the sum of squared deviations, d recomputed ----
    acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (unsigned p0 = 0; p0 < n; p0 += kStatSlots) {
        const unsigned p = p0 + slot;
        float d[4];
        depthwise(min(p, n - 1), d);
        const bool live = p < n;
        const float ex = d[0] - mean.x, ey = d[1] - mean.y, ez = d[2] - mean.z, ew = d[3] - mean.w;
        acc.x += live ? ex * ex : 0.f; acc.y += live ? ey * ey : 0.f; acc.z += live ? ez * ez : 0.f; acc.w += live ? ew * ew : 0.f;
    }
    const float4 ss = stat_sum(acc, L[1], P[1], tid);

    if (slot == 0 && c0 < Ch) {
        float4 sc, sh;
        sc.x = 1.0f / sqrtf(ss.x * inv_n + g.eps);
        sc.y = 1.0f / sqrtf(ss.y * inv_n + g.eps);
        sc.z = 1.0f / sqrtf(ss.z * inv_n + g.eps);
        sc.w = 1.0f / sqrtf(ss.w * inv_n + g.eps);
        sh.x = -mean.x * sc.x; sh.y = -mean.y * sc.y; sh.z = -mean.z * sc.z; sh.w = -mean.w * sc.w;
        const size_t o = ((size_t)img * 2 + br) * Ch + c0;
        store_out4(g.out_sc + o, sc);
        store_out4(g.out_sh + o, sh);
    }
}

}  // namespace sige

using namespace sige;

// the two separable entry points behind one set of checks; `images`: the dense form over the images of the current edit batch,
// in_scale / in_shift [E][2][Ch]
static int sep_entry(const float *actv, int tiled, int T, int H, int W, int Ch, const float *dw_weight, const float *dw_bias,
                     const float *in_scale, const float *in_shift, const float *pw_weight, const float *pw_bias, int oc, float *out,
                     void *stream, bool images) {
    if (T < 0 || H <= 0 || W <= 0 || Ch <= 0 || oc <= 0) return SIGE_HIP_EINVAL;
    if (!dw_weight || !dw_bias || !in_scale || !in_shift || !pw_weight || !pw_bias) return SIGE_HIP_EINVAL;
    if (Ch % 4 || Ch < kSepMinCh || Ch > kSepMaxCh || oc % 4 || oc < kSepMinOc || oc > kSepMaxOc) return SIGE_HIP_EUNSUPPORTED;
    if (tiled ? (H != 6 || W != 6) : T != 1) return SIGE_HIP_EUNSUPPORTED;
    const int img_shift = tiled ? 0 : stacked_shift(H);
    // (the plain dense form pads at the border of the whole tensor only; the per-image form needs stacked_shift's power-of-two height)
    if (images ? img_shift < 0 : img_shift != 0) return SIGE_HIP_EUNSUPPORTED;
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!al(actv) || !al(dw_weight) || !al(dw_bias) || !al(in_scale) || !al(in_shift) || !al(pw_weight) || !al(pw_bias) || !al(out))
        return SIGE_HIP_EUNSUPPORTED;
    if (tiled && T == 0) return SIGE_HIP_OK;
    if (!actv || !out) return SIGE_HIP_EINVAL;
    const long npix = tiled ? (long)T * 16 : (long)H * W;
    if (npix > 0x7fffffffL / 2) return SIGE_HIP_EUNSUPPORTED;
    const long npb = (npix + 15) / 16;
    const int ncb = ceil_div(oc, 16);
    const int mb_shift = ncb >= 4 ? 0 : ncb >= 2 ? 1 : 2;
    const long gx = (npb + (1 << mb_shift) - 1) >> mb_shift;
    const int gy = ceil_div(ncb, 4 >> mb_shift);
    if (gy > 65535) return SIGE_HIP_EUNSUPPORTED;
    SepArgs a = {};
    a.a = actv; a.dw_w = dw_weight; a.dw_b = dw_bias; a.sc = in_scale; a.sh = in_shift; a.pw_w = pw_weight; a.pw_b = pw_bias;
    a.out = out; a.npb = npb; a.H = H; a.W = W; a.Ch = Ch; a.oc = oc; a.mb_shift = mb_shift;
    a.img_shift = img_shift; a.aff_stride = img_shift ? 2 * Ch : 0;  // (one image: shift 0, one affine)
    const dim3 grid((unsigned)gx, (unsigned)gy, 2);
    hipStream_t st = as_stream(stream);
    return tiled ? sep_launch<true>(a, grid, st) : sep_launch<false>(a, grid, st);
}

extern "C" int sige_hip_spade_separable_nhwc_f32(const float *actv, int tiled, int T, int H, int W, int Ch,
                                                 const float *dw_weight, const float *dw_bias,
                                                 const float *in_scale, const float *in_shift,
                                                 const float *pw_weight, const float *pw_bias, int oc, float *out, void *stream) {
    SIGE_PLAN_HOOK_FIXED(sige_hip_spade_separable_nhwc_f32, actv, tiled, T, H, W, Ch, dw_weight, dw_bias, in_scale, in_shift, pw_weight, pw_bias,
                   oc, out, stream);
    return sep_entry(actv, tiled, T, H, W, Ch, dw_weight, dw_bias, in_scale, in_shift, pw_weight, pw_bias, oc, out, stream, false);
}

extern "C" int sige_hip_spade_separable_images_nhwc_f32(const float *actv, int H, int W, int Ch,
                                                        const float *dw_weight, const float *dw_bias,
                                                        const float *in_scale, const float *in_shift,
                                                        const float *pw_weight, const float *pw_bias, int oc, float *out, void *stream) {
    SIGE_PLAN_HOOK(sige_hip_spade_separable_images_nhwc_f32, actv, H, W, Ch, dw_weight, dw_bias, in_scale, in_shift, pw_weight, pw_bias, oc, out,
                   stream);
    return sep_entry(actv, 0, 1, H, W, Ch, dw_weight, dw_bias, in_scale, in_shift, pw_weight, pw_bias, oc, out, stream, true);
}

extern "C" int sige_hip_spade_separable_stats_nhwc_f32(const float *actv, int H, int W, int Ch, const float *dw_weight,
                                                       const float *dw_bias, float eps, float *out_scale, float *out_shift,
                                                       void *stream) {
    SIGE_PLAN_HOOK(sige_hip_spade_separable_stats_nhwc_f32, actv, H, W, Ch, dw_weight, dw_bias, eps, out_scale, out_shift, stream);
    if (H <= 0 || W <= 0 || Ch <= 0 || !(eps >= 0.f)) return SIGE_HIP_EINVAL;
    if (!dw_weight || !dw_bias) return SIGE_HIP_EINVAL;
    if (Ch % 4 || Ch < kSepMinCh || Ch > kSepMaxCh) return SIGE_HIP_EUNSUPPORTED;
    const int s = stacked_shift(H);
    if (s < 0) return SIGE_HIP_EUNSUPPORTED;
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!al(actv) || !al(dw_weight) || !al(dw_bias) || !al(out_scale) || !al(out_shift)) return SIGE_HIP_EUNSUPPORTED;
    if (!actv || !out_scale || !out_shift) return SIGE_HIP_EINVAL;  // (the tensors last, as in the launch above)
    const int h = s ? 1 << s : H, E = s ? H >> s : 1;
    if ((long)h * W > 0x7fffffffL / 2 || E > 65535) return SIGE_HIP_EUNSUPPORTED;
    SepStatsArgs a = {};
    a.a = actv; a.dw_w = dw_weight; a.dw_b = dw_bias; a.out_sc = out_scale; a.out_sh = out_shift;
    a.h = h; a.W = W; a.Ch = Ch; a.eps = eps;
    spade_separable_stats_kernel<<<dim3((unsigned)ceil_div(Ch, 16), 2, (unsigned)E), 256, 0, as_stream(stream)>>>(a);
    return launch_status();
}
