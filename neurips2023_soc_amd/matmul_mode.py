"""The arithmetic mode of a forward ("split": f32 products as six bf16 MFMA products of an exact three-way operand split;
"f32": the f32-input MFMA path).  hot_ops.py re-exports every name here; the routing rules that depend on the mode are in
linear_routes.py."""
from __future__ import annotations

import contextlib as _contextlib
import os as _os
import threading as _threading

# "split" (default): the layers linear_routes names run on the bf16 matrix cores (K20 / K13b / K23 / K24); "f32": every GEMM
# stays on the f32 MFMA path (K13 / K12 / library), i.e. the round-2 arithmetic.  bench.py reports both.
#
# The mode is NOT process state: it belongs to a model (SOC.matmul_mode) and reaches the ops through a thread-local that the
# model's forward sets for its own duration (use_matmul_mode), and it reaches the C ABI as an argument of each launch.  Two
# models with different modes can therefore run from two threads of one process (tests/test_gpu_forward.py).  The environment
# variable only supplies the default a model is built with.
DEFAULT_MATMUL_MODE = _os.environ.get("SOC_MATMUL", "split")
_mode_tls = _threading.local()


def matmul_mode() -> str:
    """The arithmetic of the calling thread's current forward: "split" or "f32"."""
    return getattr(_mode_tls, "mode", None) or DEFAULT_MATMUL_MODE


@_contextlib.contextmanager
def use_matmul_mode(mode):
    """`with use_matmul_mode("f32"):` -- the ops called from THIS thread inside the block run in that arithmetic (None =
    leave it as it is).  Nests; other threads are unaffected."""
    if mode is None:
        yield
        return
    if mode not in ("split", "f32"):
        raise ValueError(f"matmul mode {mode!r}: expected 'split' or 'f32'")
    prev = getattr(_mode_tls, "mode", None)
    _mode_tls.mode = mode
    try:
        yield
    finally:
        _mode_tls.mode = prev


def split_enabled() -> bool:
    return matmul_mode() == "split"


_SPLIT_OFF = frozenset(filter(None, _os.environ.get("SOC_SPLIT_OFF", "").split(",")))


def split_off(site: str) -> bool:
    """Debugging: SOC_SPLIT_OFF (a comma list, read once at import) forces a call site or kernel back to the f32 path --
    k1, k13, k24, mlp, w256, or a K20 site of linear_routes (swin, gelu, relu, multi, mul, res, add, plain)."""
    return site in _SPLIT_OFF


def k1_split_enabled() -> bool:
    """K1 (full 8x7x7 windows) on the bf16 matrix cores with the exact three-way split; SOC_SPLIT_OFF=k1 or
    SOC_MATMUL=f32 keep the f32-input MFMA form."""
    return split_enabled() and not split_off("k1")


def k13_split_enabled() -> bool:
    return split_enabled() and not split_off("k13")
