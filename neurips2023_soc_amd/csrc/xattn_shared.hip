// K3s: K3's attention core (xattn.hip) for ONE set of projected query rows and the keys / values of E expressions --
// the `vlf` blocks of a video whose frames are shared by several referring expressions (include/soc_hip_xattn_shared.h).
//
// K3 is HBM-bound on its q / out rows (tens of thousands of pixel rows against <= ~20 words).  Called once per expression
// it reads the same q rows E times; here a workgroup reads its q rows once and keeps them in registers while it walks the
// expressions, so the traffic is (1 + E) row sets instead of 2 E.  Mapping, as K3's many-query form:
//   * one lane = one query row of one head (the scaled q row and the 32-wide accumulator live in registers);
//   * one wave = 64 queries x one head; a workgroup = 4 waves = 256 queries of one head = one tile;
//   * per expression the head's K and V rows (Lk <= 64: 2 x Lk x 128 B) are staged in LDS with coalesced loads and the
//     key loops read them as broadcast ds_reads (every lane of the wave reads the same address: no bank conflict);
//   * q rows come in, and output rows go out, through a per-wave LDS tile so that a global access is 8 rows x 128 B;
//   * exact two-pass softmax, -inf padding, the arithmetic of K3's kernel line for line.
// The grid is persistent over the (query tile, head) pairs and sized from the stream's CU mask; a tile's result does not
// depend on which workgroup computes it.
#include "soc_common.h"
#include "soc_hip_xattn_shared.h"
#include <math.h>

namespace {

constexpr int HD = 32;
constexpr int KV_MAX = SOC_XATTN_SHARED_MAX_LK;
// 152 VGPRs -> three waves per SIMD = three 4-wave workgroups per CU; their LDS (36 KB tile + <= 16 KB of K / V each) fits
// the CU's 160 KB beside that
constexpr int BLOCKS_PER_CU = 3;

__global__ __launch_bounds__(256) void xattn_shared_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const uint8_t* __restrict__ kpm, float* __restrict__ out, int E, int Lq, int Lk, int H, float scale, int n_tiles) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int C = H * HD;
    __shared__ __attribute__((aligned(16))) float tile_s[4][64 * 36];
    extern __shared__ __attribute__((aligned(16))) float kv_s[];   // [2][Lk][HD]
    float* tile = tile_s[wave];
    float* Ksh = kv_s;
    float* Vsh = kv_s + Lk * HD;
    const int sub_r = lane >> 3, sub_c = lane & 7;

    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {       // block-uniform
        const int h = t % H;
        const int q0 = ((t / H) * 4 + wave) * 64;                 // first query row of this wave (may be >= Lq: clamped reads)
        __builtin_amdgcn_wave_barrier();                          // the previous tile's output rows have left the LDS tile
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = i * 8 + sub_r;
            const long qq = min(q0 + row, Lq - 1);
            const float4 x = *reinterpret_cast<const float4*>(q + qq * C + h * HD + sub_c * 4);
            *reinterpret_cast<float4*>(tile + row * 36 + sub_c * 4) = x;
        }
        __builtin_amdgcn_wave_barrier();
        float qr[HD];
#pragma unroll
        for (int i = 0; i < HD / 4; ++i) {
            const float4 x = *reinterpret_cast<const float4*>(tile + lane * 36 + 4 * i);   // same wave: no barrier needed
            qr[4 * i] = x.x * scale; qr[4 * i + 1] = x.y * scale;
            qr[4 * i + 2] = x.z * scale; qr[4 * i + 3] = x.w * scale;
        }

        for (int e = 0; e < E; ++e) {
            const float* kb = k + ((long)e * Lk) * C + h * HD;
            const float* vb = v + ((long)e * Lk) * C + h * HD;
            __syncthreads();                                      // every wave is done with the previous K / V image
            for (int idx = threadIdx.x; idx < Lk * 8; idx += 256) {
                const int j = idx >> 3, c = idx & 7;
                *reinterpret_cast<float4*>(Ksh + j * HD + c * 4) = *reinterpret_cast<const float4*>(kb + (long)j * C + c * 4);
                *reinterpret_cast<float4*>(Vsh + j * HD + c * 4) = *reinterpret_cast<const float4*>(vb + (long)j * C + c * 4);
            }
            __syncthreads();
            const uint8_t* mp = kpm ? kpm + (long)e * Lk : nullptr;

            // pass 1: row maximum over the unpadded keys
            float mx = -INFINITY;
            for (int j = 0; j < Lk; ++j) {
                if (mp && mp[j]) continue;  // wave-uniform
                const float* kr = Ksh + j * HD;
                float s = 0.f;
#pragma unroll
                for (int d = 0; d < HD; ++d) s += qr[d] * kr[d];
                mx = fmaxf(mx, s);
            }
            // pass 2: exp / accumulate
            float acc[HD];
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = 0.f;
            float l = 0.f;
            for (int j = 0; j < Lk; ++j) {
                if (mp && mp[j]) continue;
                const float* kr = Ksh + j * HD;
                const float* vr = Vsh + j * HD;
                float s = 0.f;
#pragma unroll
                for (int d = 0; d < HD; ++d) s += qr[d] * kr[d];
                const float p = __expf(s - mx);
                l += p;
#pragma unroll
                for (int d = 0; d < HD; ++d) acc[d] += p * vr[d];
            }
            const float inv = 1.f / l;  // l == 0 (all keys padded) -> NaN, as torch.softmax gives
            __builtin_amdgcn_wave_barrier();                      // the previous expression's rows have left the LDS tile
#pragma unroll
            for (int i = 0; i < HD / 4; ++i)
                *reinterpret_cast<float4*>(tile + lane * 36 + 4 * i) =
                    make_float4(acc[4 * i] * inv, acc[4 * i + 1] * inv, acc[4 * i + 2] * inv, acc[4 * i + 3] * inv);
            __builtin_amdgcn_wave_barrier();
            float* ob = out + ((long)e * Lq) * C + h * HD;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = i * 8 + sub_r;
                if (q0 + row < Lq)
                    *reinterpret_cast<float4*>(ob + (long)(q0 + row) * C + sub_c * 4) =
                        *reinterpret_cast<const float4*>(tile + row * 36 + sub_c * 4);
            }
        }
    }
}

}  // namespace

extern "C" int soc_xattn_shared_q_f32(const float* q, const float* k, const float* v, const uint8_t* key_pad_mask,
                                      float* out, int E, int Lq, int Lk, int n_heads, int head_dim, void* stream) {
    if (!q || !k || !v || !out || E <= 0 || Lq <= 0 || Lk <= 0 || n_heads <= 0) return SOC_EINVAL;
    if (head_dim != HD || Lk > KV_MAX) return SOC_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const long tiles = (long)soc_ceil_div(Lq, 256) * n_heads;
    if (tiles > 0x7fffffffL) return SOC_EUNSUPPORTED;
    long blocks = (long)soc_num_cus(st) * BLOCKS_PER_CU;      // CUs the launch stream may use
    if (blocks > tiles) blocks = tiles;
    if (blocks < 1) blocks = 1;
    const float scale = (float)sqrt(1.0 / (double)head_dim);
    hipLaunchKernelGGL(xattn_shared_kernel, dim3((unsigned)blocks), dim3(256), (size_t)2 * Lk * HD * sizeof(float), st,
                       q, k, v, key_pad_mask, out, E, Lq, Lk, n_heads, scale, (int)tiles);
    return soc_check_launch();
}
