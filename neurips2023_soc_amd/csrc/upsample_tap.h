// The per-pixel arithmetic of K6 (upsample_threshold.hip) and K6b (upsample_threshold_bits.hip): bilinear up-sampling with
// align_corners = False, restating torch's upsample_bilinear2d (scale = in / out, src = max(scale * (dst + 0.5) - 0.5, 0),
// second tap clamped to the last row / column), and the threshold.  ONE float expression for both kernels: a byte of K6 and
// a bit of K6b of the same pixel are the same comparison of the same value.
//
// "The same value" must not hang on how the compiler contracts a * b + c in each kernel (left free, it fused a different
// term per unrolled pixel of K6): contraction is switched off in here, the source coordinate is an explicit fma, and the
// four-tap sum is plain multiplies and adds, each rounded once -- whatever way they are later vectorised.
#pragma once
#include <hip/hip_runtime.h>

// the two source rows of output row y and their weights
struct soc_up_rows {
    const float* r0;
    const float* r1;
    float ly0, ly1;
};

__device__ __forceinline__ soc_up_rows soc_up_rows_of(const float* __restrict__ frame, int y, int h, int w, float sy) {
#pragma clang fp contract(off)
    const float fy = fmaxf(__fmaf_rn(sy, (float)y + 0.5f, -0.5f), 0.f);
    const int y1 = (int)fy;
    const int yp = (y1 < h - 1) ? 1 : 0;
    soc_up_rows r;
    r.ly1 = fy - (float)y1;
    r.ly0 = 1.f - r.ly1;
    r.r0 = frame + (long)y1 * w;
    r.r1 = r.r0 + (long)yp * w;
    return r;
}

// up-sampled logit of output column x (any x >= 0: the taps are clamped to the row) > thr
__device__ __forceinline__ bool soc_up_pixel_above(const soc_up_rows& r, int x, int w, float sx, float thr) {
#pragma clang fp contract(off)
    const float fx = fmaxf(__fmaf_rn(sx, (float)x + 0.5f, -0.5f), 0.f);
    int x1 = (int)fx;
    x1 = x1 < w - 1 ? x1 : w - 1;
    const int xp = (x1 < w - 1) ? 1 : 0;
    const float lx1 = fx - (float)x1, lx0 = 1.f - lx1;
    const float v = r.ly0 * (lx0 * r.r0[x1] + lx1 * r.r0[x1 + xp]) + r.ly1 * (lx0 * r.r1[x1] + lx1 * r.r1[x1 + xp]);
    return v > thr;
}
