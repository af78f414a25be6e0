/*
 * soc_hip_xattn_shared.h -- K3s, the shared-query attention core of libsoc_hip.so: K3 (soc_xattn_f32 of soc_hip.h) for ONE
 * set of projected query rows against the keys / values of E expressions.  An addition beside soc_hip.h, whose entry set
 * and ABI number it leaves alone: a library without this symbol is an older build.
 */
#ifndef SOC_HIP_XATTN_SHARED_H
#define SOC_HIP_XATTN_SHARED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOC_XATTN_SHARED_MAX_LK 64      /* K3's KV_LDS_MAX: one head's K and V rows of an expression live in LDS */

/*
 * K3s: the attention core of `vlf` for one clip and E expressions of it.
 *   q             [Lq, n_heads * 32] float32, projected pixel rows -- the same for every expression.
 *   k, v          [E, Lk, n_heads * 32] float32, projected word rows of each expression.
 *   key_pad_mask  [E, Lk] uint8 (non-zero = padded key), or NULL.
 *   out           [E, Lq, n_heads * 32] float32; every element written, nothing else.
 * DEFINITION: out[e] is what soc_xattn_f32(q, k[e], v[e], key_pad_mask[e], NULL, 1, out[e], Lq, Lk, 1, n_heads, 32,
 * batch_first = 1, ...) writes: q scaled by 1/sqrt(32), an exact two-pass softmax over the unpadded keys, padded keys at
 * weight 0 (an expression whose keys are all padded gives NaN rows, as torch.softmax does).  The expressions do not
 * influence each other.  A q row is read from memory once, not E times: the workgroup keeps its rows in registers and
 * walks the expressions, staging each one's K / V head rows in LDS.
 * Returns SOC_OK, or (soc_hip.h's codes) SOC_EINVAL: a null q, k, v or out, E <= 0, Lq <= 0, Lk <= 0 or n_heads <= 0;
 * SOC_EUNSUPPORTED: head_dim != 32 or Lk > SOC_XATTN_SHARED_MAX_LK -- the host then calls K3 once per expression.
 * Stateless, no workspace; inputs are borrowed; one launch on `stream` (a hipStream_t), whose grid follows the stream's
 * CU mask.  The result does not depend on the grid.
 */
int soc_xattn_shared_q_f32(const float* q, const float* k, const float* v, const uint8_t* key_pad_mask, float* out, int E,
                           int Lq, int Lk, int n_heads, int head_dim, void* stream);

#ifdef __cplusplus
}
#endif
#endif
