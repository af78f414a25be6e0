"""K3s (include/soc_hip_xattn_shared.h): K3's attention core for ONE set of projected query rows and E expressions.

    out = mha_core_shared_q(q, k, v, n_heads, key_padding_mask)        q [Lq,C], k / v [E,Lk,C] -> [E,Lq,C]

out[e] is what hot_ops.mha_core(q[None], k[e:e+1], v[e:e+1], n_heads, mask[e:e+1], batch_first=True) gives; the q rows are read
from memory once.  A shape the kernel refuses (more than 64 keys, a head width other than 32) is computed by K3, once per
expression -- the same kernel family, not another implementation.

Bound here and not in _lib.py, as K6b is in packed_masks.py: include/soc_hip.h, _lib.EXPORTS and the ABI number describe the
entry set of ABI 16 and stay as they are; a libsoc_hip.so without the symbol is a stale build and raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib

ENTRY = "soc_xattn_shared_q_f32"
MAX_LK = 64                                         # SOC_XATTN_SHARED_MAX_LK
_SIGNATURE = [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p]
launches = 0          # calls of the entry made through this module
fallbacks = 0         # calls the entry refused (SOC_EUNSUPPORTED) and K3 computed per expression


def _entry():
    lib = _lib.load()
    fn = getattr(lib, ENTRY, None)
    if fn is None:
        raise _lib.SocHipError(f"libsoc_hip.so does not export {ENTRY}: a stale library from before the shared-video path; "
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


def shared_q_raw(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kpm: Optional[torch.Tensor], out: torch.Tensor,
                 n_heads: int, head_dim: int) -> int:
    """The entry itself on contiguous float32 / uint8 device tensors; returns its code (tests read SOC_EUNSUPPORTED here)."""
    from . import hot_ops
    E, Lk = int(k.shape[0]), int(k.shape[1])
    return _call(q.data_ptr(), k.data_ptr(), v.data_ptr(), None if kpm is None else kpm.data_ptr(), out.data_ptr(),
                 E, int(q.shape[0]), Lk, int(n_heads), int(head_dim), hot_ops._stream())


def mha_core_shared_q(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, n_heads: int,
                      key_padding_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K3s.  q [Lq,C] projected query rows shared by the expressions, k / v [E,Lk,C] projected, key_padding_mask [E,Lk] bool
    (True = padded) -> [E,Lq,C]."""
    global fallbacks
    from . import hot_ops
    hot_ops._need_gpu(q, k, v, key_padding_mask)
    if q.dim() != 2 or k.dim() != 3 or k.shape != v.shape or k.shape[-1] != q.shape[-1]:
        raise _lib.SocHipError(f"mha_core_shared_q: expected q [Lq,C] and k, v [E,Lk,C], got {tuple(q.shape)}, "
                               f"{tuple(k.shape)}, {tuple(v.shape)}")
    q, k, v = hot_ops._f32c(q), hot_ops._f32c(k), hot_ops._f32c(v)
    (Lq, Cw), (E, Lk, _) = q.shape, k.shape
    if key_padding_mask is not None and tuple(key_padding_mask.shape) != (E, Lk):
        raise _lib.SocHipError(f"mha_core_shared_q: key_padding_mask {tuple(key_padding_mask.shape)} is not [E,Lk] = {(E, Lk)}")
    kpm = None if key_padding_mask is None else hot_ops._as_u8(key_padding_mask)
    out = torch.empty((E, Lq, Cw), dtype=torch.float32, device=q.device)
    with hot_ops._timed("xattn_shared", ((1 + E) * q.numel() + k.numel() + v.numel()) * 4):
        code = shared_q_raw(q, k, v, kpm, out, n_heads, Cw // n_heads)
    if code == _lib.SOC_EUNSUPPORTED:
        fallbacks += 1
        for e in range(E):
            out[e] = hot_ops.mha_core(q[None], k[e:e + 1], v[e:e + 1], n_heads,
                                      None if key_padding_mask is None else key_padding_mask[e:e + 1], batch_first=True)[0]
        return out
    _lib.check(code, ENTRY)
    return out
