/*
 * soc_hip_center_bits.h -- K6c, the centre-frame mask entry of libsoc_hip.so: the post-processing of the A2D-Sentences /
 * JHMDB-Sentences protocol (reference models/postprocessing.py:10-55) and the pixel counts its metrics need
 * (metrics.py:27-60), for all queries of a batch of samples in one launch.  An addition beside soc_hip.h, whose entry set and
 * ABI number it leaves alone: a library without this symbol is an older build.
 */
#ifndef SOC_HIP_CENTER_BITS_H
#define SOC_HIP_CENTER_BITS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOC_CENTER_BITS_MAX 64     /* most samples of one call: their geometry travels as kernel arguments */

/*
 * K6c: N samples (annotated frames), Q queries each.  The mask of sample n, query q at the sample's ORIGINAL size is what the
 * reference's four ops give: bilinear up-sampling of the [h, w] logits to the padded model input Hp x Wp (align_corners =
 * False), sigmoid > 0.5, crop to the resized size rh x rw, nearest-neighbour resize to oh x ow.  Per output pixel (y, x):
 *     sy = min((int)floorf(y * ((float)rh / (float)oh)), rh - 1), sx likewise from rw and ow        (the nearest step)
 *     bit = K6's tap (csrc/upsample_tap.h) at pixel (sy, sx) of the Hp x Wp grid, logit > 0          (the bilinear step)
 * The crop is implicit: sy < rh, sx < rw.
 *   logits      float32 [N, Q, h, w] on the device, contiguous.
 *   rh, rw, oh, ow   N host ints each: resized (before padding) and original size of every sample; samples of one call may
 *               differ in them.  1 <= rh <= Hp, 1 <= rw <= Wp.  Read during the call, they travel to the kernel as arguments:
 *               no device allocation, no synchronisation, nothing remembered.
 *   out         nullable.  The packed mask (soc_hip_bits.h: RB = SOC_BITS_ROW_BYTES(ow_n) bytes per row) of sample n, query q
 *               is the [oh_n, RB] bytes at out + out_offset[n] + q * oh_n * RB; out and every out_offset[n] (N host longs,
 *               bytes, >= 0) are multiples of 8.  Every byte of every plane is written, padding bits as zero.  With
 *               out == NULL no mask is stored (the counts-only mode of the metrics path) and out_offset is not read.
 *   gt_bits     nullable.  The ground truth of sample n is ONE packed plane [oh_n, RB] at gt_bits + gt_offset[n] (N host
 *               longs, bytes, >= 0; pointer and offsets multiples of 8).  Bits at x >= ow_n may hold anything: they influence
 *               no count.  Borrowed, never written.
 *   counts      int32 [N, Q, 3] = (inter, pred_area, gt_area) of every (sample, query) against the sample's ground truth;
 *               required when gt_bits is given, nullable otherwise (given without gt_bits: inter = gt_area = 0).  Every
 *               element is written by the call -- the caller does not zero it.  Integer arithmetic only, summed in one fixed
 *               order: the result does not depend on the launch geometry or the run.
 * Decided before any launch (soc_hip.h's codes): a negative N or Q, a non-positive h, w, Hp or Wp, a null pointer with work
 * to do (logits, a size list, out_offset with out, gt_offset with gt_bits, counts with gt_bits, out and counts both null), a
 * pointer or offset that is not a multiple of 8 or negative, a size outside 1..rh <= Hp / 1..rw <= Wp, oh or ow < 1
 * -> SOC_EINVAL;  N > SOC_CENTER_BITS_MAX, Q > 65535, oh or ow > 65535 -> SOC_EUNSUPPORTED.
 * N == 0 or Q == 0: SOC_OK, nothing is launched.  Inputs are borrowed, the one launch goes to `stream` (a hipStream_t).
 */
int soc_center_frame_bits(const float* logits, int N, int Q, int h, int w, int Hp, int Wp, const int* rh, const int* rw,
                          const int* oh, const int* ow, uint8_t* out, const long* out_offset, const uint8_t* gt_bits,
                          const long* gt_offset, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
