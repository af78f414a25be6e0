// K6c (include/soc_hip_center_bits.h): the centre-frame post-processing of the A2D-Sentences / JHMDB-Sentences protocol --
// bilinear up-sampling to the padded input size, threshold, crop, nearest-neighbour resize to the original size -- for all
// Q queries of N samples in one launch, as packed masks (soc_hip_bits.h) and / or the integer counts the metrics need.
//
// One block per (sample, query) plane, sixteen waves; a wave takes every sixteenth 64-bit word of the plane.  One lane per
// output pixel: the lane maps its pixel to its source pixel (sy, sx) of the padded grid (the nearest step, torch's float
// arithmetic) and evaluates K6's tap there, so a bit of K6c and a bit of K6b at the same pixel of the padded grid are the
// same comparison of the same value.  The wave's ballot IS the output word (lanes at x >= ow vote 0: padding bits are zeros
// written by the same store as the data); its popcounts, and those of the ground-truth word it meets, are wave-uniform
// integers.  Each wave keeps its three sums, the block adds the sixteen in wave order and stores the plane's row of `counts`
// with plain stores: no atomics, nothing to zero, one fixed order of summation.
//
// A source pixel that several output pixels share (oh > rh or ow > rw) is evaluated once per output pixel, not staged: the
// sharing lanes are neighbours in x or the same lanes of a neighbouring row, their four taps hit the same cache lines, and
// the tap is ~20 VALU operations -- less than a barrier per row would cost.  The evaluation protocol resizes DOWN to the
// original size (JHMDB: 320 x 426 -> 240 x 320), where no source pixel is needed twice.
#include "soc_common.h"
#include "soc_hip_bits.h"
#include "soc_hip_center_bits.h"
#include "upsample_tap.h"

namespace {

constexpr int WAVES = 16;

struct Samples {                       // per-sample geometry: kernel arguments (2 KiB at the cap)
    int rh[SOC_CENTER_BITS_MAX], rw[SOC_CENTER_BITS_MAX], oh[SOC_CENTER_BITS_MAX], ow[SOC_CENTER_BITS_MAX];
    long out_off[SOC_CENTER_BITS_MAX], gt_off[SOC_CENTER_BITS_MAX];
};

// torch's nearest source index: min((int)floorf(dst * scale), in - 1) with scale = (float)in / (float)out
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
#pragma clang fp contract(off)
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}

__global__ __launch_bounds__(WAVES* SOC_WAVE) void center_frame_bits_kernel(
    const float* __restrict__ logits, uint8_t* __restrict__ out, const uint8_t* __restrict__ gt_bits,
    int32_t* __restrict__ counts, const Samples s, int Q, int h, int w, float up_y, float up_x) {
    __shared__ int partial[WAVES][3];
    const int plane = blockIdx.x;                      // n * Q + q
    const int n = plane / Q, q = plane - n * Q;
    const int wave = threadIdx.x / SOC_WAVE, lane = threadIdx.x & (SOC_WAVE - 1);
    const int rh = s.rh[n], rw = s.rw[n], oh = s.oh[n], ow = s.ow[n];
    const int words = SOC_BITS_ROW_BYTES(ow) / 8;
    const int total = oh * words;                      // <= 65535 * 1024
    const float ny = (float)rh / (float)oh, nx = (float)rw / (float)ow;
    const float* frame = logits + (long)plane * h * w;
    unsigned long long* dst =
        out ? reinterpret_cast<unsigned long long*>(out + s.out_off[n]) + (long)q * total : nullptr;
    const unsigned long long* gt =
        gt_bits ? reinterpret_cast<const unsigned long long*>(gt_bits + s.gt_off[n]) : nullptr;
    int inter = 0, area = 0, gt_area = 0;
    for (int i = wave; i < total; i += WAVES) {        // uniform over the wave
        const int y = i / words, k = i - y * words;
        const int x = k * SOC_WAVE + lane;
        const soc_up_rows rows = soc_up_rows_of(frame, nearest_src(y, ny, rh), h, w, up_y);
        const bool on = x < ow && soc_up_pixel_above(rows, nearest_src(x, nx, rw), w, up_x, 0.f);
        const unsigned long long bits = __ballot(on);
        if (dst && lane == 0) dst[i] = bits;
        if (counts) {
            const int valid = ow - k * SOC_WAVE;       // >= 1: pixels of the row inside this word
            const unsigned long long keep = valid >= SOC_WAVE ? ~0ull : ((1ull << valid) - 1ull);
            const unsigned long long g = gt ? (gt[i] & keep) : 0ull;
            inter += __popcll(bits & g);
            area += __popcll(bits);
            gt_area += __popcll(g);
        }
    }
    if (!counts) return;                               // uniform over the block
    if (lane == 0) {
        partial[wave][0] = inter;
        partial[wave][1] = area;
        partial[wave][2] = gt_area;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int sum = 0;
        for (int v = 0; v < WAVES; ++v) sum += partial[v][threadIdx.x];
        counts[(long)plane * 3 + threadIdx.x] = sum;
    }
}

}  // namespace

extern "C" int soc_center_frame_bits(const float* logits, int N, int Q, int h, int w, int Hp, int Wp, const int* rh,
                                     const int* rw, const int* oh, const int* ow, uint8_t* out, const long* out_offset,
                                     const uint8_t* gt_bits, const long* gt_offset, int32_t* counts, void* stream) {
    if (N < 0 || Q < 0 || h <= 0 || w <= 0 || Hp <= 0 || Wp <= 0) return SOC_EINVAL;
    if (N == 0 || Q == 0) return SOC_OK;
    if (!logits || !rh || !rw || !oh || !ow) return SOC_EINVAL;
    if ((!out && !counts) || (out && !out_offset) || (gt_bits && (!gt_offset || !counts))) return SOC_EINVAL;
    if ((((uintptr_t)out) & 7) != 0 || (((uintptr_t)gt_bits) & 7) != 0) return SOC_EINVAL;
    if (N > SOC_CENTER_BITS_MAX || Q > 65535) return SOC_EUNSUPPORTED;
    Samples s = {};
    for (int n = 0; n < N; ++n) {
        if (rh[n] < 1 || rh[n] > Hp || rw[n] < 1 || rw[n] > Wp || oh[n] < 1 || ow[n] < 1) return SOC_EINVAL;
        if (out && (out_offset[n] < 0 || (out_offset[n] & 7) != 0)) return SOC_EINVAL;
        if (gt_bits && (gt_offset[n] < 0 || (gt_offset[n] & 7) != 0)) return SOC_EINVAL;
        if (oh[n] > 65535 || ow[n] > 65535) return SOC_EUNSUPPORTED;
        s.rh[n] = rh[n], s.rw[n] = rw[n], s.oh[n] = oh[n], s.ow[n] = ow[n];
        s.out_off[n] = out ? out_offset[n] : 0;
        s.gt_off[n] = gt_bits ? gt_offset[n] : 0;
    }
    hipLaunchKernelGGL(center_frame_bits_kernel, dim3(N * Q), dim3(WAVES * SOC_WAVE), 0, (hipStream_t)stream, logits, out,
                       gt_bits, counts, s, Q, h, w, (float)h / (float)Hp, (float)w / (float)Wp);
    return soc_check_launch();
}
