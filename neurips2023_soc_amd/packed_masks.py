"""Bit-packed masks (include/soc_hip_bits.h): one bit per output pixel from the kernel to the PNG file.

Format: a packed mask is uint8 [..., H0, RB] with RB = row_bytes(W0) = 8 * ceil(W0 / 64) -- every row starts on a 64-bit
word -- and pixel x of a row is bit x % 8 of byte x // 8 (little bit order: np.packbits(mask, axis=-1, bitorder="little"),
zero-padded to RB).  Bits at positions >= W0 are zero when K6b or pack() wrote them; unpack() and the PNG encoder
(png_fast.encode_bits) ignore them whatever they hold.

K6b, `soc_upsample_threshold_bits`, is bound here and not in _lib.py: include/soc_hip.h, _lib.EXPORTS and the ABI number
describe the entry set of ABI 16 and stay as they are; a libsoc_hip.so without the symbol is a stale build and raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

ENTRY = "soc_upsample_threshold_bits"
_SIGNATURE = [C.c_void_p, C.c_long, C.c_void_p] + [C.c_int] * 6 + [C.c_float, C.c_void_p]
launches = 0          # calls of the entry made through this module (tests count launches per group with it)


def row_bytes(W0: int) -> int:
    """Bytes per packed row of W0 pixels: whole 64-bit words."""
    return 8 * (-(-int(W0) // 64))


def _entry():
    """K6b of the handle _lib.load() returns, with its ctypes signature set on first sight."""
    lib = _lib.load()
    fn = getattr(lib, ENTRY, None)
    if fn is None:
        raise _lib.SocHipError(f"libsoc_hip.so does not export {ENTRY}: a stale library from before the packed-mask path; "
                               "rebuild it with `python -m neurips2023_soc_amd.build_ext --force`")
    if getattr(fn, "argtypes", ()) is None:          # a ctypes function nobody has described yet
        fn.restype = C.c_int
        fn.argtypes = list(_SIGNATURE)
    return fn


def _call(*args) -> int:
    """Every argument goes over as its ctypes type, so a proxy in front of the library (tests.guarded.record_lib_calls hands
    out closures, which carry no argtypes) passes the same values as the bound function."""
    global launches
    launches += 1
    return int(_entry()(*[t(a) for t, a in zip(_SIGNATURE, args)]))


def upsample_threshold_bits(logits: torch.Tensor, size: Sequence[int], threshold_logit: float = 0.0,
                            clip_stride: Optional[int] = None, clips: int = 1) -> torch.Tensor:
    """K6b.  One clip: logits [T,h,w] float32 -> uint8 [T,H0,RB].  A group: logits [B,T,h,w], a view whose clips are
    `stride(0)` elements apart and contiguous inside (e.g. cut out of a [B,R] record), or a [T,h,w] view of the FIRST clip
    with `clips` = B and `clip_stride` = the distance in elements -> uint8 [B,T,H0,RB], one launch.  Every bit equals the
    bool hot_ops.upsample_threshold gives for that pixel; padding bits are zero."""
    from . import hot_ops
    hot_ops._need_gpu(logits)
    if logits.dtype != torch.float32:
        raise _lib.SocHipError(f"expected float32, got {logits.dtype}")
    grouped = logits.dim() == 4
    if grouped:
        if clips != 1 and clips != logits.shape[0]:
            raise _lib.SocHipError("clips disagrees with the leading dimension of the logits")
        B, (T, h, w) = int(logits.shape[0]), logits.shape[1:]
        inner_ok = logits[0].is_contiguous() if B else True
        if not inner_ok or (B > 1 and logits.stride(0) < T * h * w):
            logits = logits.contiguous()
        stride = int(logits.stride(0)) if B > 1 else T * h * w
        if clip_stride is not None and B > 1 and int(clip_stride) != stride:
            raise _lib.SocHipError("clip_stride disagrees with the stride of the [B,T,h,w] logits")
    else:
        if logits.dim() != 3:
            raise _lib.SocHipError(f"expected [T,h,w] or [B,T,h,w] logits, got {tuple(logits.shape)}")
        B, (T, h, w) = int(clips), logits.shape
        if not logits.is_contiguous():
            if B != 1:
                raise _lib.SocHipError("the first clip's [T,h,w] view must be contiguous when clips > 1")
            logits = logits.contiguous()
        stride = T * h * w if clip_stride is None else int(clip_stride)
        grouped = B != 1 or clip_stride is not None
    H0, W0 = int(size[0]), int(size[1])
    out = torch.empty((B, T, H0, row_bytes(W0)) if grouped else (T, H0, row_bytes(W0)), dtype=torch.uint8, device=logits.device)
    with hot_ops._timed("upsample_threshold_bits", B * T * h * w * 4 + out.numel()):
        code = _call(logits.data_ptr(), stride, out.data_ptr(), B, int(T), int(h), int(w), H0, W0, float(threshold_logit),
                     hot_ops._stream())
    _lib.check(code, ENTRY)
    return out


def pack(mask):
    """bool / 0-1 mask [..., H0, W0] (torch on any device, or numpy) -> packed uint8 [..., H0, row_bytes(W0)] of the same kind,
    padding bits zero.  The CPU reference of the format; on a device tensor it runs as a handful of torch ops."""
    if isinstance(mask, torch.Tensor):
        W0 = mask.shape[-1]
        padded = torch.zeros(*mask.shape[:-1], row_bytes(W0) * 8, dtype=torch.uint8, device=mask.device)
        padded[..., :W0] = mask != 0
        weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=mask.device)
        return (padded.view(*mask.shape[:-1], row_bytes(W0), 8).to(torch.int32) * weights).sum(-1).to(torch.uint8)
    m = np.asarray(mask) != 0
    W0 = m.shape[-1]
    out = np.zeros(m.shape[:-1] + (row_bytes(W0),), np.uint8)
    bits = np.packbits(m, axis=-1, bitorder="little")
    out[..., :bits.shape[-1]] = bits
    return out


def unpack(bits, W0: int):
    """packed uint8 [..., H0, >= ceil(W0 / 8)] (torch or numpy) -> bool [..., H0, W0]; bits at positions >= W0 are ignored."""
    W0 = int(W0)
    if isinstance(bits, torch.Tensor):
        if bits.dtype != torch.uint8 or bits.shape[-1] * 8 < W0:
            raise ValueError(f"unpack: expected uint8 [..., >= {-(-W0 // 8)}], got {bits.dtype} {tuple(bits.shape)}")
        shifts = torch.arange(8, dtype=torch.uint8, device=bits.device)
        b = bits[..., :-(-W0 // 8)]
        return ((b[..., None] >> shifts) & 1).view(*b.shape[:-1], b.shape[-1] * 8)[..., :W0].to(torch.bool)
    a = np.asarray(bits)
    if a.dtype != np.uint8 or a.shape[-1] * 8 < W0:
        raise ValueError(f"unpack: expected uint8 [..., >= {-(-W0 // 8)}], got {a.dtype} {a.shape}")
    return np.unpackbits(a[..., :-(-W0 // 8)], axis=-1, bitorder="little")[..., :W0].astype(bool)
