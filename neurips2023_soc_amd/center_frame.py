"""K6c (include/soc_hip_center_bits.h): the masks of the centre-frame protocol (A2D-Sentences / JHMDB-Sentences) at original
size, bit-packed (packed_masks.py), and the integer counts its metrics need -- all queries of a batch of samples, one launch.

    bits, counts = center_frame_bits(logits, padded, resized, original, gt_bits=..., masks=True)

plus the host side of the format: uncompressed COCO run lengths from packed bits (rle_counts) and back (rle_decode).

Bound here and not in _lib.py, as K6b is in packed_masks.py: include/soc_hip.h, _lib.EXPORTS and the ABI number describe the
entry set of ABI 16 and stay as they are; a libsoc_hip.so without the symbol is a stale build and raises.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .packed_masks import row_bytes, unpack

ENTRY = "soc_center_frame_bits"
MAX_SAMPLES = 64                                    # SOC_CENTER_BITS_MAX: samples of one call
_SIGNATURE = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 10
launches = 0          # calls of the entry made through this module (the driver's tests count calls per batch with it)


def _entry():
    lib = _lib.load()
    fn = getattr(lib, ENTRY, None)
    if fn is None:
        raise _lib.SocHipError(f"libsoc_hip.so does not export {ENTRY}: a stale library from before the centre-frame path; "
                               "rebuild it with `python -m neurips2023_soc_amd.build_ext --force`")
    if getattr(fn, "argtypes", ()) is None:          # a ctypes function nobody has described yet
        fn.restype = C.c_int
        fn.argtypes = list(_SIGNATURE)
    return fn


def _call(*args) -> int:
    """Every argument goes over as its ctypes type (see packed_masks._call)."""
    global launches
    launches += 1
    return int(_entry()(*[t(a) for t, a in zip(_SIGNATURE, args)]))


def _array(ctype, values: Sequence[int]):
    values = [int(v) for v in values]
    return (ctype * max(len(values), 1))(*values)


def plane_bytes(size: Sequence[int]) -> int:
    """Bytes of one packed mask of `size` = (oh, ow)."""
    return int(size[0]) * row_bytes(size[1])


def mask_offsets(original: Sequence[Sequence[int]], Q: int) -> Tuple[List[int], int]:
    """(byte offset of every sample's [Q, oh, RB] block in the flat mask buffer center_frame_bits returns, its total size)."""
    offsets, at = [], 0
    for size in original:
        offsets.append(at)
        at += int(Q) * plane_bytes(size)              # RB is a multiple of 8: every offset is
    return offsets, at


def pack_ground_truth(masks: Sequence, device) -> Tuple[torch.Tensor, List[int]]:
    """Per-sample ground-truth masks [oh_n, ow_n] (numpy or torch, non-zero = foreground) -> (one flat uint8 device buffer of
    their packed planes, the byte offset of each)."""
    from .packed_masks import pack
    planes = [np.ascontiguousarray(pack(np.asarray(m) != 0)).reshape(-1) for m in masks]
    offsets, at = [], 0
    for p in planes:
        offsets.append(at)
        at += p.size
    flat = np.concatenate(planes) if planes else np.zeros(0, np.uint8)
    return torch.from_numpy(flat).to(device), offsets


def center_frame_bits(logits: torch.Tensor, padded: Sequence[int], resized: Sequence[Sequence[int]],
                      original: Sequence[Sequence[int]], gt_bits: Optional[torch.Tensor] = None,
                      gt_offsets: Optional[Sequence[int]] = None, masks: bool = True, counts: Optional[bool] = None):
    """K6c.  logits float32 [N,Q,h,w] on the device: the mask logits of N annotated frames; padded = (Hp, Wp) of the model
    input they belong to; resized[n] = (rh, rw) before padding, original[n] = (oh, ow).  gt_bits: a flat uint8 device buffer
    holding one packed ground-truth plane [oh_n, RB] per sample at gt_offsets[n] bytes (pack_ground_truth makes both).
    -> (bits, counts):
      bits    (masks=True) flat uint8 buffer; sample n's packed masks [Q, oh_n, RB] start at mask_offsets(original, Q)[0][n]
              -- sample_masks() cuts them out; None with masks=False, the counts-only mode (no mask is ever stored).
      counts  int32 [N,Q,3] = (inter, pred_area, gt_area); made when gt_bits is given or counts=True, else None.
    N above MAX_SAMPLES goes through in chunks of MAX_SAMPLES samples, one launch each."""
    from . import hot_ops
    hot_ops._need_gpu(logits)
    if logits.dtype != torch.float32 or logits.dim() != 4:
        raise _lib.SocHipError(f"center_frame_bits: expected float32 [N,Q,h,w] logits, got {logits.dtype} {tuple(logits.shape)}")
    logits = logits.contiguous()
    N, Q, h, w = (int(v) for v in logits.shape)
    if len(resized) != N or len(original) != N:
        raise _lib.SocHipError(f"center_frame_bits: {N} samples but {len(resized)} resized and {len(original)} original sizes")
    want_counts = (gt_bits is not None) if counts is None else bool(counts)
    if gt_bits is not None:
        hot_ops._need_gpu(gt_bits)
        if gt_bits.dtype != torch.uint8 or not gt_bits.is_contiguous() or gt_offsets is None or len(gt_offsets) != N:
            raise _lib.SocHipError("center_frame_bits: gt_bits must be a contiguous uint8 buffer with one offset per sample")
        if not want_counts:
            raise _lib.SocHipError("center_frame_bits: a ground truth is only read for the counts")
    if not masks and not want_counts:
        raise _lib.SocHipError("center_frame_bits: nothing to produce (masks=False and no counts)")
    offsets, total = mask_offsets(original, Q)
    bits = torch.empty(total, dtype=torch.uint8, device=logits.device) if masks else None
    cnt = torch.empty((N, Q, 3), dtype=torch.int32, device=logits.device) if want_counts else None
    for n0 in range(0, N, MAX_SAMPLES):
        n1 = min(N, n0 + MAX_SAMPLES)
        sel = slice(n0, n1)
        geo = [_array(C.c_int, [s[i] for s in seq[sel]]) for seq in (resized, original) for i in (0, 1)]   # rh, rw, oh, ow
        out_off = _array(C.c_long, offsets[sel])
        gt_off = _array(C.c_long, gt_offsets[sel] if gt_bits is not None else [])
        moved = (n1 - n0) * Q * h * w * 4 + (sum(Q * plane_bytes(s) for s in original[sel]) if masks else 0)
        with hot_ops._timed("center_frame_bits", moved):
            code = _call(logits[n0:n1].data_ptr(), n1 - n0, Q, h, w, int(padded[0]),
                         int(padded[1]), *[C.addressof(g) for g in geo],
                         bits.data_ptr() if masks and total else None, C.addressof(out_off) if masks else None,
                         gt_bits.data_ptr() if gt_bits is not None else None,
                         C.addressof(gt_off) if gt_bits is not None else None,
                         cnt[n0:n1].data_ptr() if want_counts and Q else None, hot_ops._stream())
        _lib.check(code, ENTRY)
    return bits, cnt


def sample_masks(bits: torch.Tensor, original: Sequence[Sequence[int]], Q: int, n: int) -> torch.Tensor:
    """Sample n's packed masks, uint8 [Q, oh, RB] (a view), out of center_frame_bits' flat buffer."""
    offsets, _ = mask_offsets(original, Q)
    oh, ow = (int(v) for v in original[n])
    return bits[offsets[n]:offsets[n] + Q * plane_bytes((oh, ow))].view(Q, oh, row_bytes(ow))


# ---------------------------------------------------------------------------------------------------------------------
# uncompressed COCO run lengths (the `counts` list of a COCO RLE: column-major runs, the first one of zeros)

def rle_counts(bits, size: Sequence[int]) -> List[int]:
    """One packed mask [oh, RB] (numpy or a CPU tensor) of `size` = (oh, ow) -> the run lengths of mask.flatten(order="F"),
    starting with the run of zeros (0 when the first pixel is set)."""
    oh, ow = int(size[0]), int(size[1])
    flat = np.asarray(unpack(np.asarray(bits), ow)).reshape(oh, ow).flatten(order="F")
    if flat.size == 0:
        return []
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate(([0], change, [flat.size]))
    runs = np.diff(edges).tolist()
    return ([0] + runs) if flat[0] else runs


def rle_decode(counts: Sequence[int], size: Sequence[int]) -> np.ndarray:
    """The inverse of rle_counts: bool [oh, ow]."""
    oh, ow = int(size[0]), int(size[1])
    values = np.zeros(len(counts), bool)
    values[1::2] = True
    flat = np.repeat(values, np.asarray(counts, dtype=np.int64))
    if flat.size != oh * ow:
        raise ValueError(f"run lengths cover {flat.size} pixels, the mask has {oh * ow}")
    return flat.reshape(ow, oh).T
