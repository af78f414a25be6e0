// K25: multi-head self-attention core for short sequences (L <= 64 tokens), one workgroup per (batch, head).
//
// Replaces torch.nn.functional.scaled_dot_product_attention as HuggingFace's RobertaSelfAttention calls it for the text encoder
// SOC.forward_text runs per clip (reference models/soc.py:167-181: RobertaModel on the tokenised expression; 12 layers x 12 heads
// x 64 dims, 10-32 tokens).  PyTorch dispatches that call to its AOTriton `attn_fwd` kernel -- the one compiled-by-Triton kernel
// that was left in the timed graph (VERDICT r3 "missing" #6).  The problem is tiny and latency-bound (12 launches per clip on the
// text branch, beside Video-Swin): a 256-thread workgroup per (batch, head) with Q, K and V of the head in LDS ([LP][D + 4]
// floats, LP = L rounded up to 16, pad rows zero).  Both products run on the f32 matrix instruction (v_mfma_f32_16x16x4_f32: f32
// operands, f32 accumulation -- no splitting needed at this size), a wave per 16 x 16 tile: S = Q K^T tile by tile into LDS, a
// quad of lanes per row for the softmax (two-pass, as the reference's), then O = P V tile by tile.  An MFMA's four k-lanes take the
// dims (keys) 16 s + 4 g + e of float4 reads, the same permutation on both operands, so every LDS read of Q / K / P is a
// conflict-free ds_read_b128.  q / k / v / out are token-major [B, L, H * D] (what the projections produce: no transposes),
// the mask is additive ([B, 1, Lq | 1, Lk] with the given strides, -inf on padding) or NULL.
#include "soc_common.h"

namespace {

constexpr int NT = 256;
typedef float f32x4 __attribute__((ext_vector_type(4)));

// value of lane ^ 1 (CTRL 0xB1: quad_perm 1,0,3,2) or lane ^ 2 (0x4E: quad_perm 2,3,0,1) -- one DPP move, no LDS crossbar
template <int CTRL>
__device__ __forceinline__ float quad_xor(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
}

template <int D>
__global__ __launch_bounds__(NT) void small_attn_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                        const float* __restrict__ v, const float* __restrict__ mask,
                                                        float* __restrict__ out, int L, int H, float scale, long mask_b,
                                                        long mask_q) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int RS = D + 4;                       // row stride: rows r = 0..15 of a float4 column on 16 distinct bank quads
    constexpr int D4 = D / 4;
    const int LT = (L + 15) >> 4, LP = LT * 16;
    const int PS = LP + 4;                          // 20 / 36 / 52 / 68 floats: the same property for the P rows
    float* Qs = lds;                                // [LP][RS]
    float* Ks = Qs + LP * RS;                       // [LP][RS]
    float* Vs = Ks + LP * RS;                       // [LP][RS]
    float* Ps = Vs + LP * RS;                       // [LP][PS] scores, then probabilities (columns >= L: 0)
    float* Ms = Ps + LP * PS;                       // mask of this batch element: [L] (key mask) or [L][L]
    const int b = blockIdx.x / H, h = blockIdx.x % H, t = threadIdx.x;
    const long E = (long)H * D;
    const long base = (long)b * L * E + (long)h * D;
    {   // every global load of the workgroup is issued before the first LDS store: one memory round trip
        constexpr int ITERS = (64 * D4 + NT - 1) / NT;
        float4 qq[ITERS], kk[ITERS], vv[ITERS];
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int i = t + NT * it, row = i / D4, c = i % D4;
            qq[it] = make_float4(0.f, 0.f, 0.f, 0.f); kk[it] = qq[it]; vv[it] = qq[it];
            if (row < L) {
                const long g = base + (long)row * E + 4 * c;
                qq[it] = *reinterpret_cast<const float4*>(q + g);
                kk[it] = *reinterpret_cast<const float4*>(k + g);
                vv[it] = *reinterpret_cast<const float4*>(v + g);
            }
        }
        const int nm = mask ? (mask_q ? L * L : L) : 0;
        const float m0 = t < nm ? mask[(long)b * mask_b + (mask_q ? (long)(t / L) * mask_q + t % L : t)] : 0.f;
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int i = t + NT * it, row = i / D4, c = i % D4;
            if (row < LP) {
                *reinterpret_cast<float4*>(Qs + row * RS + 4 * c) = qq[it];
                *reinterpret_cast<float4*>(Ks + row * RS + 4 * c) = kk[it];
                *reinterpret_cast<float4*>(Vs + row * RS + 4 * c) = vv[it];
            }
        }
        if (t < nm) Ms[t] = m0;
        for (int i = t + NT; i < nm; i += NT) Ms[i] = mask[(long)b * mask_b + (long)(i / L) * mask_q + i % L];   // [L][L], L > 16
    }
    __syncthreads();
    const int lane = t & 63, wave = t >> 6, r = lane & 15, g = lane >> 4;
    // ---- S = Q K^T * scale + mask: tile (ti, tj), accumulator register i = S[16 ti + 4 g + i][16 tj + r]
    for (int tile = wave; tile < LT * LT; tile += NT / 64) {
        const int ti = tile / LT, tj = tile % LT;
        const float* qr = Qs + (16 * ti + r) * RS + 4 * g;
        const float* kr = Ks + (16 * tj + r) * RS + 4 * g;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < D / 16; ++s) {
            const float4 a = *reinterpret_cast<const float4*>(qr + 16 * s);
            const float4 c = *reinterpret_cast<const float4*>(kr + 16 * s);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, c.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, c.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, c.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, c.w, acc, 0, 0, 0);
        }
        const int j = 16 * tj + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int qi = 16 * ti + 4 * g + i;
            float sv = acc[i] * scale;
            if (mask && qi < L && j < L) sv += Ms[mask_q ? qi * L + j : j];
            Ps[qi * PS + j] = sv;
        }
    }
    __syncthreads();
    {   // softmax: 4 lanes per row, LP / 4 consecutive keys each (float4 reads), quad reductions on the DPP path
        const int row = t >> 2, part = t & 3, j0 = part * 4 * LT;
        float* pr = Ps + row * PS + j0;
        float4 sc[4];
        float mx = -INFINITY;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            sc[s] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            if (s < LT && row < L) {
                const float4 x = *reinterpret_cast<const float4*>(pr + 4 * s);
                const int j = j0 + 4 * s;
                sc[s].x = j < L ? x.x : -INFINITY; sc[s].y = j + 1 < L ? x.y : -INFINITY;
                sc[s].z = j + 2 < L ? x.z : -INFINITY; sc[s].w = j + 3 < L ? x.w : -INFINITY;
            }
            mx = fmaxf(fmaxf(mx, fmaxf(sc[s].x, sc[s].y)), fmaxf(sc[s].z, sc[s].w));
        }
        mx = fmaxf(mx, quad_xor<0xB1>(mx));
        mx = fmaxf(mx, quad_xor<0x4E>(mx));
        float sum = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {               // a fully masked row gives zeros, not NaN
            sc[s].x = mx == -INFINITY ? 0.f : __expf(sc[s].x - mx); sc[s].y = mx == -INFINITY ? 0.f : __expf(sc[s].y - mx);
            sc[s].z = mx == -INFINITY ? 0.f : __expf(sc[s].z - mx); sc[s].w = mx == -INFINITY ? 0.f : __expf(sc[s].w - mx);
            sum += (sc[s].x + sc[s].y) + (sc[s].z + sc[s].w);
        }
        sum += quad_xor<0xB1>(sum);
        sum += quad_xor<0x4E>(sum);
        const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s < LT && row < L)
                *reinterpret_cast<float4*>(pr + 4 * s) = make_float4(sc[s].x * inv, sc[s].y * inv, sc[s].z * inv, sc[s].w * inv);
    }
    __syncthreads();
    // ---- O = P V: tile (ti, td), accumulator register i = O[16 ti + 4 g + i][16 td + r]; rows >= L are never stored
    for (int tile = wave; tile < LT * (D / 16); tile += NT / 64) {
        const int ti = tile / (D / 16), td = tile % (D / 16);
        const float* pr = Ps + (16 * ti + r) * PS + 4 * g;
        const float* vc = Vs + (4 * g) * RS + 16 * td + r;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < LT; ++s) {
            const float4 a = *reinterpret_cast<const float4*>(pr + 16 * s);
            const float* vr = vc + 16 * s * RS;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, vr[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, vr[RS], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, vr[2 * RS], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, vr[3 * RS], acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int qi = 16 * ti + 4 * g + i;
            if (qi < L) out[base + (long)qi * E + 16 * td + r] = acc[i];
        }
    }
}

}  // namespace

extern "C" int soc_small_attn_f32(const float* q, const float* k, const float* v, const float* mask, float* out, int B, int L,
                                  int H, int D, float scale, long mask_batch_stride, long mask_query_stride, void* stream) {
    if (B < 0 || L < 0 || H <= 0) return SOC_EINVAL;
    if (B == 0 || L == 0) return SOC_OK;
    if (!q || !k || !v || !out) return SOC_EINVAL;
    if (L > 64 || (D != 32 && D != 64)) return SOC_EUNSUPPORTED;
    if ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) != 0) return SOC_EUNSUPPORTED;
    const int LP = (L + 15) / 16 * 16;
    const size_t lds = ((size_t)3 * LP * (D + 4) + (size_t)LP * (LP + 4) + (size_t)(mask ? (mask_query_stride ? L * L : L) : 0)) * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    if (lds > 64 * 1024) {                                 // L > 48 at D = 64: above the default dynamic-LDS limit
        if (soc_allow_lds<small_attn_kernel<64>>(96 * 1024) != SOC_OK || soc_allow_lds<small_attn_kernel<32>>(96 * 1024) != SOC_OK)
            return SOC_ELAUNCH;
    }
    if (D == 64)
        hipLaunchKernelGGL(small_attn_kernel<64>, dim3((unsigned)(B * H)), dim3(NT), lds, st, q, k, v, mask, out, L, H, scale,
                           mask_batch_stride, mask_query_stride);
    else
        hipLaunchKernelGGL(small_attn_kernel<32>, dim3((unsigned)(B * H)), dim3(NT), lds, st, q, k, v, mask, out, L, H, scale,
                           mask_batch_stride, mask_query_stride);
    return soc_check_launch();
}
