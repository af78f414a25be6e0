/*
 * soc_hip_bits.h -- the bit-packed mask format and K6b, the entry of libsoc_hip.so that writes it.  An addition beside
 * soc_hip.h (whose entry set and ABI number it leaves alone): a library without this symbol is an older build.
 *
 * PACKED MASK FORMAT (used by K6b, soc_png_encode_bits of soc_host.h, neurips2023_soc_amd/packed_masks.py)
 *   A packed mask is [N, H0, RB] uint8 with RB = 8 * ceil(W0 / 64): every row starts on a 64-bit word.
 *   Pixel x of a row is bit (x % 8) of byte (x / 8) -- little bit order: what a wave64 ballot stored as a little-endian
 *   64-bit word gives, and what np.packbits(mask, axis=-1, bitorder="little"), zero-padded to RB bytes per row, gives.
 *   Bits at positions >= W0 of a row are written as zero by K6b.  Consumers do not rely on that: they mask them.
 */
#ifndef SOC_HIP_BITS_H
#define SOC_HIP_BITS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes per packed row of W0 pixels */
#define SOC_BITS_ROW_BYTES(W0) (8 * (((W0) + 63) / 64))

/*
 * K6b: K6 (soc_upsample_threshold_u8: bilinear up-sampling, align_corners = False, fused with `logit > threshold_logit`)
 * with one BIT per output pixel, for B clips in one launch.
 *   logits  float32; frame t of clip b is the contiguous [h, w] image at logits + b * clip_stride + t * h * w (elements).
 *           A [n, R] record of a group replay, with each clip's mask logits at one offset of its row, is read in place:
 *           logits = row 0's mask logits, clip_stride = R.
 *   out     [B, T, H0, RB] uint8, contiguous, 8-byte aligned; every byte of it is written, padding bits as zero.
 * Every bit equals the byte K6 writes for the same pixel: both kernels evaluate the same device function.
 * Returns SOC_OK, or (soc_hip.h's codes) SOC_EINVAL: a negative B or T, a non-positive size, a null pointer with work to
 * do, `out` not 8-byte aligned, clip_stride < T * h * w with B > 1;  SOC_EUNSUPPORTED: B * T > 65535 or H0 > 65535.
 * B == 0 or T == 0: SOC_OK, nothing is launched.  Inputs are borrowed, the launch goes to `stream` (a hipStream_t).
 */
int soc_upsample_threshold_bits(const float* logits, long clip_stride, uint8_t* out, int B, int T, int h, int w, int H0,
                                int W0, float threshold_logit, void* stream);

#ifdef __cplusplus
}
#endif
#endif
