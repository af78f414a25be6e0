// K6b: K6 (upsample_threshold.hip) with one bit per output pixel -- the packed mask format of include/soc_hip_bits.h -- and
// B clips per launch, each read where a group replay's record holds it (clip_stride elements apart): one launch per group,
// T * H0 * RB bytes per clip leave the chip instead of T * H0 * W0.
//
// One lane per output pixel, one wave per 64-bit word of a row: the wave's ballot IS the word (lane i = pixel 64 k + i = bit
// i), lane 0 stores it.  Lanes at x >= W0 vote 0, so the padding bits are zeros written by the same store as the data.
// A block is four waves = four consecutive words of one row; RB * 8 is a multiple of 64, so a wave is either wholly inside
// the padded row or wholly outside it (and leaves before the ballot).
#include "soc_common.h"
#include "soc_hip_bits.h"
#include "upsample_tap.h"

namespace {

__global__ __launch_bounds__(256) void upsample_threshold_bits_kernel(
    const float* __restrict__ logits, long clip_stride, unsigned long long* __restrict__ out, int T, int h, int w, int H0,
    int W0, int words, float sy, float sx, float thr) {
    const int bt = blockIdx.z;                       // clip b, frame t
    const int y = blockIdx.y;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int word = x >> 6;                         // uniform over the wave
    if (word >= words) return;
    const int b = bt / T, t = bt - b * T;
    const soc_up_rows rows = soc_up_rows_of(logits + (long)b * clip_stride + (long)t * h * w, y, h, w, sy);
    const bool on = x < W0 && soc_up_pixel_above(rows, x, w, sx, thr);
    const unsigned long long bits = __ballot(on);
    if ((threadIdx.x & (SOC_WAVE - 1)) == 0) out[((long)bt * H0 + y) * words + word] = bits;
}

}  // namespace

extern "C" int soc_upsample_threshold_bits(const float* logits, long clip_stride, uint8_t* out, int B, int T, int h, int w,
                                           int H0, int W0, float threshold_logit, void* stream) {
    if (B < 0 || T < 0 || h <= 0 || w <= 0 || H0 <= 0 || W0 <= 0) return SOC_EINVAL;
    if (B == 0 || T == 0) return SOC_OK;
    if (!logits || !out || (((uintptr_t)out) & 7) != 0) return SOC_EINVAL;
    if (B > 1 && clip_stride < (long)T * h * w) return SOC_EINVAL;
    if ((long)B * T > 65535 || H0 > 65535) return SOC_EUNSUPPORTED;
    const int words = SOC_BITS_ROW_BYTES(W0) / 8;
    dim3 grid(soc_ceil_div(words, 4), H0, B * T);
    hipLaunchKernelGGL(upsample_threshold_bits_kernel, grid, dim3(256), 0, (hipStream_t)stream, logits, clip_stride,
                       reinterpret_cast<unsigned long long*>(out), T, h, w, H0, W0, words, (float)h / (float)H0,
                       (float)w / (float)W0, threshold_logit);
    return soc_check_launch();
}
