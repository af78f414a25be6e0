/*
 * soc_hip_jf_bits.h -- K27b, the per-expression J&F counting entry of libsoc_hip.so: K27 (soc_davis_jf_counts_u8 of
 * soc_hip.h) for predictions that are already bit-packed masks (soc_hip_bits.h).  An addition beside soc_hip.h, whose entry
 * set and ABI number it leaves alone: a library without these symbols is an older build.
 *
 * FORMAT IDENTITY.  A packed mask row (soc_hip_bits.h) is RB = 8 * ceil(W / 64) bytes, pixel x = bit x % 8 of byte x / 8.
 * Read as ceil(W / 64) little-endian 64-bit words that is bit x % 64 of word x / 64 -- the plane layout K27 builds from
 * label maps.  K6b's output [B, T, H0, RB] is therefore E = B prediction planes that K27b reads where they lie.
 */
#ifndef SOC_HIP_JF_BITS_H
#define SOC_HIP_JF_BITS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOC_JF_BITS_MAX 255        /* most expressions, and most distinct objects, of one call */

/*
 * K27b: one video -- E expressions, T frames of H x W, O distinct ground-truth objects -- scored in one call.
 *   gt_labels  [T, H, W] uint8 on the device; 255 is void when use_void != 0.
 *   obj_ids    O host ints, the distinct object labels used, each in 1..254.  A label that occurs in no frame is legal: its
 *              ground truth is empty everywhere.
 *   exp_obj    E host ints, expression e is scored against object obj_ids[exp_obj[e]]; several expressions may name one
 *              object.  Both lists are read during the call and travel to the kernels as arguments: no device allocation,
 *              no synchronisation, nothing remembered.
 *   pred_bits  expression e is the packed mask [T, H, RB] at pred_bits + e * exp_stride (bytes), on the device.  pred_bits
 *              and exp_stride are multiples of 8.  Bits at x >= W may hold anything: they influence no count.  Borrowed,
 *              never written, never expanded to bytes.
 *   counts     [E, T, 6] int32 = (inter, union, n_fg, n_gt, fg_match, gt_match), every element written: exactly the row K27
 *              gives with pairs == 0 for gt = (gt_labels == obj_ids[exp_obj[e]]) against fg = plane e, a void pixel
 *              belonging to neither; _seg2bmap and the disk dilation of `radius` as K27 documents them in soc_hip.h.
 *   workspace  device memory, 8-byte aligned.  soc_jf_bits_workspace_bytes returns the bytes of ONE frame's planes (three
 *              planes for each of the O + E masks), the minimum; the call goes through the frames in chunks of as many as
 *              the workspace it is given holds.  The counts do not depend on the chunking.  The query returns 0 for sizes
 *              the call refuses.
 * The ground-truth mask, boundary and dilated planes are built once per object and frame, whatever the number of
 * expressions that name the object.
 * Decided before any launch: a null pointer, a non-positive E, O, T, H or W, pred_bits or exp_stride not a multiple of 8
 * -> SOC_EINVAL; radius outside [0, 64], E or O above 255, an exp_obj outside [0, O), an id outside 1..254,
 * H * W >= 2^31, exp_stride < T * H * RB -> SOC_EUNSUPPORTED; a workspace shorter than one frame -> SOC_EWORKSPACE
 * (soc_hip.h's codes).  Integer arithmetic only: the result does not depend on the launch geometry or the run.
 */
size_t soc_jf_bits_workspace_bytes(int E, int O, int H, int W);
int soc_jf_counts_bits(const uint8_t* gt_labels, const uint8_t* pred_bits, long exp_stride, const int* obj_ids,
                       const int* exp_obj, int32_t* counts, int E, int O, int T, int H, int W, int radius, int use_void,
                       void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
