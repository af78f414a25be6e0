// Arithmetic shared by the kernels that run f32 products on the bf16 matrix cores (exact three-way operand split; DESIGN.md
// section 3): the split itself, the six-product MFMA group, the exact-erf GELU with its constants in VGPRs.
#pragma once
#include <hip/hip_runtime.h>

namespace soc_split {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// A constant that must live in a VGPR.  Measured on MI355X (tools/experiments/pk_mfma_probe.hip): while a wave that mixes
// bf16 MFMAs with LDS traffic is resident, packed f32 instructions (v_pk_fma_f32 ...) with an SGPR source return wrong low
// halves in lanes 48..63.  Left alone the compiler feeds literal constants (the GELU polynomial, 1 / C, eps) to packed
// instructions from SGPR pairs; passed through this opaque v_mov they stay vector operands (DESIGN.md section 3;
// tests/test_isa_rules.py checks the generated code of every kernel file that uses these helpers).
__device__ __forceinline__ float in_vgpr(float c) {
    float r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(c));
    return r;
}

struct GeluK { float rs2, a0, one, c5, c4, c3, c2, c1, nlog2e, half; };
__device__ __forceinline__ GeluK gelu_k() {
    return {in_vgpr(0.70710678118654752f), in_vgpr(0.3275911f), in_vgpr(1.0f), in_vgpr(1.061405429f), in_vgpr(-1.453152027f),
            in_vgpr(1.421413741f), in_vgpr(-0.284496736f), in_vgpr(0.254829592f), in_vgpr(-1.4426950408889634f),
            in_vgpr(0.5f)};
}
// exact (erf) GELU as nn.GELU() computes it: 0.5 x (1 + erf(x / sqrt 2)), erf by Abramowitz & Stegun 7.1.26 (|err| <= 1.5e-7,
// ~1 ulp of the 1 + erf it is added to), branch-free (libm's erff is piecewise); K13 (ws_linear.hip) has the f32 original
__device__ __forceinline__ float gelu_erf(float x, const GeluK& k) {
    const float z = fabsf(x) * k.rs2;
    const float t = __builtin_amdgcn_rcpf(fmaf(k.a0, z, k.one));
    float p = fmaf(k.c5, t, k.c4);
    p = fmaf(p, t, k.c3);
    p = fmaf(p, t, k.c2);
    p = fmaf(p, t, k.c1);
    const float e = __builtin_amdgcn_exp2f(z * z * k.nlog2e);
    const float erf_abs = fmaf(-p * t, e, k.one);
    const float half = k.half * x;
    return fmaf(half, copysignf(erf_abs, x), half);
}

// f32 x 8 -> three bf16 x 8 with h0 + h1 + h2 == v exactly (8 + 8 + 8 significand bits, round to nearest at each level)
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& h0, bf16x8& h1, bf16x8& h2) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const __bf16 a0 = (__bf16)v[i];
        const float r1 = v[i] - (float)a0;
        const __bf16 a1 = (__bf16)r1;
        const float r2 = r1 - (float)a1;
        h0[i] = a0; h1[i] = a1; h2[i] = (__bf16)r2;
    }
}

// acc += a . b with a = wa[0] + wa[1] + wa[2], b = xb0 + xb1 + xb2: six of the nine products, smallest first; the three
// dropped ones are <= 2^-23 |a b|
__device__ __forceinline__ void mfma6(f32x4& acc, const bf16x8 (&wa)[3], const bf16x8& xb0, const bf16x8& xb1, const bf16x8& xb2) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[2], xb0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[1], xb1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[0], xb2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[1], xb0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[0], xb1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[0], xb0, acc, 0, 0, 0);
}

}  // namespace soc_split
