// Do subnormal fp16 operands arrive in v_mfma_f32_16x16x32_f16 (gfx950), and does the fp32 -> fp16 conversion the compiler emits
// (v_cvt_pk_f16_f32) produce them?  One MFMA per case: A[i][k] = a (every element), B[k][j] = b -> D = 32 a b if nothing is flushed.
// Cases: a = 2^-20 (an fp16 subnormal) as A against b = 1, the same as B, and a = 2^-10 (normal) as the control.  Decides whether
// csrc/attention_tokens_f16.hip NEEDS its 2^15 scaling of the probabilities (it carries it either way).
//   hipcc --offload-arch=gfx950 -O3 mfma_f16_subnormal_probe.hip -o mfma_f16_subnormal_probe && ./mfma_f16_subnormal_probe
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__global__ void k(float *o, const float *x) {
    // (the values come from memory: nothing is folded at compile time)
    const float a = x[0], b = x[1];
    const f16x8 ah = __builtin_convertvector(f32x8{a, a, a, a, a, a, a, a}, f16x8);
    const f16x8 bh = __builtin_convertvector(f32x8{b, b, b, b, b, b, b, b}, f16x8);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 d0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, z, 0, 0, 0);  // subnormal as A
    const f32x4 d1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, ah, z, 0, 0, 0);  // subnormal as B
    o[threadIdx.x] = d0[0];
    o[64 + threadIdx.x] = d1[0];
    o[128 + threadIdx.x] = (float)ah[0];  // what the conversion made of a
}
int main() {
    float *dx, *dout, r[192];
    int flushed = 0;
    hipMalloc(&dx, 2 * sizeof(float)); hipMalloc(&dout, sizeof(r));
    const float cases[2][2] = {{9.5367431640625e-07f, 1.f}, {9.765625e-04f, 1.f}};  // 2^-20, 2^-10
    for (int c = 0; c < 2; ++c) {
        hipMemcpy(dx, cases[c], 2 * sizeof(float), hipMemcpyHostToDevice);
        k<<<1, 64>>>(dout, dx);
        if (hipMemcpy(r, dout, sizeof(r), hipMemcpyDeviceToHost) != hipSuccess) { printf("hip error\n"); return 2; }
        const float want = 32.f * cases[c][0];
        printf("a = %g (%s): converted %g; as A: D = %g, as B: D = %g, unflushed D = %g\n", cases[c][0], c ? "normal fp16" : "fp16 subnormal",
               r[128], r[0], r[64], want);
        if (c == 0) flushed = (r[0] != want) + 2 * (r[64] != want) + 4 * (r[128] != cases[c][0]);
    }
    printf("subnormal fp16 operands: %s\n", flushed ? "FLUSHED somewhere (see above)" : "kept by the conversion and by both MFMA operands");
    return 0;
}
