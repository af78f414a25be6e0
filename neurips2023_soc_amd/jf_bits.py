"""K27b (include/soc_hip_jf_bits.h): the six J&F counts of K27 for predictions that are bit-packed masks (packed_masks.py).

    counts = jf_counts_bits(gt_labels, obj_ids, exp_obj, pred_bits, radius)        int32 [E,T,6]

One call scores one video: E expressions against O distinct ground-truth objects, expression e against object
obj_ids[exp_obj[e]].  The prediction planes are read where they lie -- K6b's [B,T,H0,RB] output of a launch group, or a slice
of a larger buffer -- and the ground-truth planes are built once per object, however many expressions name it.

Bound here and not in _lib.py, as K6b is in packed_masks.py: include/soc_hip.h, _lib.EXPORTS and the ABI number describe the
entry set of ABI 16 and stay as they are; a libsoc_hip.so without the symbols is a stale build and raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from .packed_masks import row_bytes

ENTRY = "soc_jf_counts_bits"
QUERY = "soc_jf_bits_workspace_bytes"
MAX_IDS = 255                                       # SOC_JF_BITS_MAX: expressions, and distinct objects, of one call
AMPLE_BYTES = 64 << 20                              # the workspace jf_counts_bits allocates holds at most this many bytes of planes
_SIGNATURE = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 7 + \
             [C.c_void_p, C.c_size_t, C.c_void_p]
_QUERY_SIGNATURE = [C.c_int] * 4
launches = 0          # calls of the entry made through this module (the driver's tests count calls per group with it)


def _fn(name: str, restype, signature):
    lib = _lib.load()
    fn = getattr(lib, name, None)
    if fn is None:
        raise _lib.SocHipError(f"libsoc_hip.so does not export {name}: a stale library from before the per-expression J&F "
                               "path; rebuild it with `python -m neurips2023_soc_amd.build_ext --force`")
    if getattr(fn, "argtypes", ()) is None:          # a ctypes function nobody has described yet
        fn.restype = restype
        fn.argtypes = list(signature)
    return fn


def workspace_bytes(E: int, O: int, H: int, W: int) -> int:
    """Bytes of ONE frame's planes, the smallest workspace the entry takes; 0 for sizes it refuses."""
    return int(_fn(QUERY, C.c_size_t, _QUERY_SIGNATURE)(*[t(int(a)) for t, a in zip(_QUERY_SIGNATURE, (E, O, H, W))]))


def _call(*args) -> int:
    """Every argument goes over as its ctypes type (see packed_masks._call)."""
    global launches
    launches += 1
    return int(_fn(ENTRY, C.c_int, _SIGNATURE)(*[t(a) for t, a in zip(_SIGNATURE, args)]))


def _int_array(values: Sequence[int]):
    values = [int(v) for v in values]
    return (C.c_int * max(len(values), 1))(*values), len(values)


def jf_counts_bits(gt_labels: torch.Tensor, obj_ids: Sequence[int], exp_obj: Sequence[int], pred_bits: torch.Tensor,
                   radius: int, use_void: bool = True, exp_stride: Optional[int] = None,
                   workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K27b.  gt_labels uint8 [T,H,W] on the device (255 = void when use_void); obj_ids: the O distinct labels scored, each in
    1..254; exp_obj: per expression an index into obj_ids.  pred_bits: uint8 [E,T,H,RB] packed masks whose expressions are
    `stride(0)` bytes apart and contiguous inside (a [B,T,H0,RB] result of K6b, a slice or a strided view of a larger
    buffer), or the [T,H,RB] view of the FIRST expression with `exp_stride` = the distance in bytes to each next one ->
    int32 [E,T,6] (inter, union, n_fg, n_gt, fg_match, gt_match): the counts hot_ops.davis_jf_counts(pairs=False) gives for a
    one-object label map per expression.  Padding bits of pred_bits may hold anything.  workspace: a uint8 device tensor of at
    least workspace_bytes(E, O, H, W) bytes to use instead of allocating one (the frames go through in chunks of what it
    holds; the counts do not depend on it)."""
    from . import hot_ops
    hot_ops._need_gpu(gt_labels, pred_bits)
    if gt_labels.dtype != torch.uint8 or gt_labels.dim() != 3 or pred_bits.dtype != torch.uint8:
        raise _lib.SocHipError("jf_counts_bits: gt_labels must be uint8 [T,H,W] and pred_bits uint8")
    gt_labels = gt_labels.contiguous()
    T, H, W = (int(v) for v in gt_labels.shape)
    RB = row_bytes(W)
    ids, O = _int_array(obj_ids)
    exps, E = _int_array(exp_obj)
    one = T * H * RB
    if pred_bits.dim() == 4:
        if tuple(pred_bits.shape) != (E, T, H, RB):
            raise _lib.SocHipError(f"jf_counts_bits: pred_bits {tuple(pred_bits.shape)} is not [E,T,H,RB] = {(E, T, H, RB)}")
        if exp_stride is not None and E > 1 and int(exp_stride) != int(pred_bits.stride(0)):
            raise _lib.SocHipError("jf_counts_bits: exp_stride disagrees with the stride of the [E,T,H,RB] masks")
        inner_ok = pred_bits[0].is_contiguous() if E else True
        stride = int(pred_bits.stride(0)) if E > 1 else one
        if not inner_ok or stride < one or stride % 8 or pred_bits.data_ptr() % 8:
            pred_bits, stride = pred_bits.contiguous(), one
            if pred_bits.data_ptr() % 8:
                pred_bits = pred_bits.clone()
    else:
        if tuple(pred_bits.shape) != (T, H, RB) or not pred_bits.is_contiguous():
            raise _lib.SocHipError(f"jf_counts_bits: expected the first expression's contiguous [T,H,RB] = {(T, H, RB)} view, "
                                   f"got {tuple(pred_bits.shape)}")
        stride = one if exp_stride is None else int(exp_stride)
    need = workspace_bytes(E, O, H, W)
    if workspace is None:
        frames = max(1, min(T, AMPLE_BYTES // need)) if need else 1
        workspace = torch.empty(max(need * frames, 8), dtype=torch.uint8, device=gt_labels.device)
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != gt_labels.device:
        raise _lib.SocHipError("jf_counts_bits: the workspace must be a contiguous uint8 tensor on the device of the masks")
    out = torch.empty((E, T, 6), dtype=torch.int32, device=gt_labels.device)
    counts = out if out.numel() else torch.empty(1, dtype=torch.int32, device=gt_labels.device)
    with hot_ops._timed("jf_counts_bits", gt_labels.numel() + E * one + out.numel() * 4):
        code = _call(gt_labels.data_ptr(), pred_bits.data_ptr(), stride, C.addressof(ids), C.addressof(exps), counts.data_ptr(),
                     E, O, T, H, W, int(radius), int(bool(use_void)), workspace.data_ptr(), int(workspace.numel()),
                     hot_ops._stream())
    _lib.check(code, ENTRY)
    return out
