"""Which kernel runs a linear layer: every preference rule of the hot path.

A pixel-sized layer goes to K7 (few rows), K12 (f32 MFMA, short reductions), K13 / K13b ("k13b": weights stationary in LDS), K20
(bf16 split, tiled), K24 (bf16 split, x split once per row tile) or the library GEMM; K23 takes a whole two-layer block.  What a
kernel CAN run is its `hot_ops.*_supported` predicate, beside its launcher; where it measured FASTER is decided here, from shapes,
dtypes, devices and the arithmetic mode alone (nothing here needs the native library): `route_linear` / `route_linear_multi` for
one layer / several layers on one input, `plan_stage` for the blocks of a Video-Swin stage.  `fused.linear` and
`video_swin.BasicLayer.forward` execute these answers, `routes.table()` prints them and tests/golden/routes.json pins them.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from . import hot_ops
from .matmul_mode import k13_split_enabled, split_enabled, split_off

LABELS = ("k7", "k12", "k13b", "k20", "k23", "k24", "library")
FLOWS = ("ws", "k20", "k23", "k24", "k5")


class Stand:
    """Stand-in for a tensor (CUDA float32 unless told otherwise): the rules read shape / dtype / device only."""

    def __init__(self, *shape: int, dtype=torch.float32, is_cuda: bool = True):
        self.shape, self.dtype, self.is_cuda = tuple(shape), dtype, is_cuda

    def numel(self) -> int:
        return math.prod(self.shape)


def split_wins(rows: int, N: int, K: int, fused_passes: int = 0, site: str = "plain") -> bool:
    """Does K20 beat the f32 path for a [rows, K] x [N, K]^T layer?  From tools/split_probe.py on MI355X (round 3): K20
    runs at 100-125 TFLOP/s f32-equivalent once the grid fills the chip and K is short, about what the tuned f32 library
    GEMM reaches, so it wins where it also removes separate passes (`fused_passes`: LayerNorm, GELU, residual / mul /
    positional adds), and loses on long-K layers with few row tiles (K >= 768 with < 30 000 rows)."""
    if not split_enabled() or K % 8 or N % 4 or rows < 1024 or split_off(site):
        return False
    if K > 768:
        # long reductions (Video-Swin stage-3 fc2 + shortcut: K = 3072; the last merging reduction: K = 1536), round 6,
        # tools/experiments/longk_probe.py: at the 19 200 rows of a ten-clip launch group K20 runs them at 180 TFLOP/s where the
        # f32 library GEMM (+ its add pass) reaches 110; a tie at 7 680 rows (four clips), a loss at one clip's 1 920 (35 against 95)
        return rows >= 12288 and N >= 512
    if rows * N < 5_500_000:                    # too few tiles to fill 256 CUs (stage-2/3 proj, stage-3 qkv, coarse levels)
        return False
    if K > 512:                                 # K = 768: only the wide, GELU-fused fc1 of stage 3 (1920 x 768 -> 3072)
        return fused_passes >= 1 and N >= 1024
    if fused_passes == 0 and rows < 16384:      # bare GEMM on a short token map: a tie at best
        return False
    return True


def _f32_on_gpu(x) -> bool:
    return x.is_cuda and x.dtype == torch.float32


def is_small(x) -> bool:
    """True when linear(x, ...) runs in K7 rather than in the library GEMM."""
    K = x.shape[-1]
    return _f32_on_gpu(x) and K % 16 == 0 and x.numel() // K <= hot_ops.SMALL_LINEAR_MAX_ROWS


def mlp_ok(x, lin1, lin2) -> bool:
    """K23 takes the whole two-layer block lin2(act(lin1(LN(x)))) (+ residual, + LayerNorm behind it): pixel-sized inputs of
    width 96 / 128 / 192 / 256 / 384 / 512 (Video-Swin stages 0-2, the deformable encoder's feed-forward block)."""
    return (lin1.bias is not None and lin2.bias is not None and x.numel() // x.shape[-1] >= 4096
            and hot_ops.mlp_split_supported(x, lin1.weight, lin2.weight))


def ws_dense_ok(x, weight) -> bool:
    """K13b's step-by-step form (K = 384 / 512, no LayerNorm in front) for a plain linear layer on a pixel-sized, already
    normalised input: Video-Swin stage 2 qkv / proj / fc1 (53 / 26 / 71 us against the library's 74 / 30 and K20's 75-80,
    tools/experiments/k13b_time.py)."""
    K = x.shape[-1]
    return (_f32_on_gpu(x) and K in (384, 512) and k13_split_enabled()
            and x.numel() // K >= 4096 and hot_ops.ws_linear_supported(x, weight, False))


def ws_plain_ok(x, weight) -> bool:
    """K13b for a linear layer outside a Video-Swin stage: the K = 384 / 512 form above, or the K = 96 / 128 / 192 / 256 form on
    a tall input (patch-merging reductions, input_proj of the finer levels)."""
    K = x.shape[-1]
    return ws_dense_ok(x, weight) or (
        _f32_on_gpu(x) and K in (96, 128, 192, 256) and k13_split_enabled()
        and x.numel() // K >= 16384 and hot_ops.ws_linear_supported(x, weight, False))


def w256_tall_ok(x, weight) -> bool:
    """256 x 256 layers at the row counts of a launch group (the encoder's value_proj / output_proj + shortcut over 385 600 rows, the
    fusion blocks' projections over 288 000): K20's tiles edge out K13b's four column ranges and K24's streamed weights there
    (round 6, tools/experiments/w256_probe.py: 335 / 378 / 346 us at 385 600 rows, 242 / 265 / 259 at 288 000; K13b keeps 73 600)."""
    return (_f32_on_gpu(x) and x.shape[-1] == 256 and tuple(weight.shape) == (256, 256)
            and x.numel() // 256 >= 200_000 and split_enabled() and not split_off("plain") and not split_off("w256")
            and hot_ops.linear_split_supported(x, weight))


def _split_ok(x, weight, fused_passes: int, site: str = "plain", ln: bool = False) -> bool:
    K = x.shape[-1]
    return (_f32_on_gpu(x) and hot_ops.linear_split_supported(x, weight, ln)
            and split_wins(x.numel() // K, weight.shape[0], K, fused_passes, site))


def xs_ok(x, weight) -> bool:
    """K24 (x split once per row tile, weights streamed) where it measured faster than K13b / K20 / the library
    (tools/experiments/k24_time.py): input widths 384 / 768 (512 / 1024 for Swin-B) on pixel-sized inputs (Video-Swin stage 2 / 3 qkv, proj, fc1, the
    patch-merging reduction into stage 2), and width 256 up to 40 960 rows (the fusion blocks' query projection, the encoder's
    value_proj / output_proj at 38 560 rows: 41 us against K13b's 47, tools/experiments/k24_main_tail.py)."""
    K = x.shape[-1]
    rows = x.numel() // K
    return (rows * weight.shape[0] >= 2_000_000 and (K in (384, 512, 768, 1024) or (K == 256 and 16384 <= rows <= 40960))
            and hot_ops.xs_linear_supported(x, weight))       # (narrow outputs on few rows: the library's small tiles win)


def route_linear(x, weight, bias=None, *, ln: bool = False, add=None, act: str = "none", mul=None, residual=None) -> str:
    """Which kernel runs mul * act(LN(x [+ add]) @ weight.T + bias) + residual: the first rule below that holds, decided from
    shapes, dtypes, devices and the mode only.  A GELU-fused layer (a Video-Swin fc1 on a normalised input) differs from the plain /
    ReLU form where it was measured differently: never K7 (which has no GELU), K13b only in its K = 384 / 512 form, no 256 x 256
    rule, and K12 in front of the library.  A LayerNorm in front (`ln`) that no stage plan covers is K20's or nobody's: the other
    rules were measured on normalised inputs only, and the library cannot take it (fused.linear raises there)."""
    K = x.shape[-1]
    rows, gelu, bare = x.numel() // K, act == "gelu", add is None and mul is None and not ln
    passes = int(ln) + int(add is not None) + int(act != "none") + int(mul is not None) + int(residual is not None)
    site = ("gelu" if gelu else "relu" if act == "relu" else "mul" if mul is not None else "res" if residual is not None
            else "add" if add is not None else "plain")
    rules = (
        ("k7", lambda: not gelu and not ln and is_small(x)),
        ("k20", lambda: not gelu and bare and w256_tall_ok(x, weight)),
        ("k24", lambda: bare and xs_ok(x, weight)),
        ("k13b", lambda: bare and (ws_dense_ok if gelu else ws_plain_ok)(x, weight)),
        ("k20", lambda: _split_ok(x, weight, passes, site, ln) and (add is None or tuple(add.shape) == tuple(x.shape))),
        ("k12", lambda: gelu and bare and residual is None and _f32_on_gpu(x) and rows >= 16384
         and K <= 256 and K % 16 == 0 and weight.shape[0] % 4 == 0),
        ("library", lambda: True),
    )
    return next(name for name, holds in rules if holds())


def route_linear_multi(x, layers, add=None) -> str:
    """Which kernel runs several layers on the same (x [+ add]): "k7" (few rows, up to four layers), "k20" (two stacked layers
    as one two-output launch, x + pos in the loader), "k12" (the f32-MFMA form of the same) or "library"."""
    if is_small(x) and len(layers) <= 4:
        return "k7"
    K = x.shape[-1]
    two_on_sum = (_f32_on_gpu(x) and len(layers) == 2 and add is not None
                  and tuple(add.shape) == tuple(x.shape) and all(u for _, _, u in layers)
                  and all(w.shape[0] % 4 == 0 for w, _, _ in layers))
    if two_on_sum and all(b is not None for _, b, _ in layers) and _split_ok(x, layers[0][0], 2, "multi"):
        return "k20"
    if two_on_sum and K % 16 == 0 and K <= 256:
        return "k12"
    return "library"


class StagePlan(NamedTuple):
    """How one Video-Swin stage runs its blocks.  `flow`:
    "ws"  norm1 + qkv | K1 | proj + shortcut | norm2 + fc1 + GELU | fc2 + shortcut as K13 launches, LayerNorms in their prologues
          (tall stages of width 96 / 128 / 192: stages 0-1 of Swin-T / -S, stage 0 of Swin-B; in the f32 mode up to 256);
    "k20" the same on K20, LayerNorm folded into the packed weights (wider tall stages: Swin-B stage 1; SOC_SPLIT_OFF=k13);
    "k24" the same on K24: stage 3 (C = 768, Swin-B 1024; fc2's input width 4 C is beyond K24);
    "k23" one LayerNorm pass at the stage's entry, then per block qkv | K1 | proj + shortcut | K23 (norm2 + MLP + shortcut +
          norm1 of the next block): stage 2 of Swin-T / -S (C = 384) and of Swin-B (C = 512);
    "k5"  every shortcut add fused with the LayerNorm that consumes it (K5), one GEMM per layer: the rest.
    qkv / proj / fc1 / fc2: route_linear's labels; mlp: "k23" where one K23 launch takes norm2 + MLP + shortcut (fc1 = fc2 = None)."""
    flow: str
    qkv: str
    proj: str
    mlp: Optional[str]
    fc1: Optional[str]
    fc2: Optional[str]


def _weight_stationary(x, blk) -> bool:
    """K13 pays where the token map is tall and the weights of a layer fit a CU's LDS in a few column ranges."""
    return (x.is_cuda and x.numel() // x.shape[-1] >= 16384
            and hot_ops.ws_linear_supported(x, blk.attn.qkv.weight, True)
            and hot_ops.ws_linear_supported(x, blk.attn.proj.weight, False)
            and hot_ops.ws_linear_supported(x, blk.mlp.fc1.weight, True))


def _split_flow(x, blk) -> bool:
    """Tall stages wider than K13's sweet spot (C >= 192: stage 1 of Swin-T / -S, stages 1 of Swin-B): every layer on
    K20 (tools/split_probe.py: 66 / 29 / 80 us against 75 / 36 / 99-108 us for K13 at Swin-T stage 1)."""
    C, rows = x.shape[-1], x.numel() // x.shape[-1]
    return (_f32_on_gpu(x) and C >= 192 and rows >= 16384
            and split_wins(rows, 3 * C, C, 1, "swin") and split_wins(rows, C, C, 1, "swin")
            and hot_ops.linear_split_supported(x, blk.attn.qkv.weight, True))


def _stage_flow(x, blk) -> str:
    C = x.shape[-1]
    qkv, proj, fc1, fc2 = blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2
    # stage 1 (C = 192) in the split arithmetic: K13b beats K20 on qkv / proj / fc1 (49 / 24 / 71 against 60 / 30 / 74 us,
    # tools/experiments/k13b_time.py); with SOC_SPLIT_OFF=k13 the K20 flow takes it
    prefer_ws = k13_split_enabled() and C in hot_ops.WS_SPLIT_LN_K and _weight_stationary(x, blk)
    # C = 384 / 512 keep the "k23" flow however many rows a launch group brings (four clips: 29 440): K24 qkv 161 us against
    # K20 + LayerNorm 229, K23 with norm1 of the next block 392 against 415 + a LayerNorm in the next qkv
    # (tools/experiments/stage2_group_flow.py); the "k20" flow is for the tall stages K24 / K23 do not cover that way
    prefer_k23 = C in (384, 512) and mlp_ok(x, fc1, fc2) and all(xs_ok(x, w) for w in (qkv.weight, proj.weight))
    if not prefer_ws and not prefer_k23 and _split_flow(x, blk):
        return "k20"
    if _weight_stationary(x, blk):
        return "ws"
    if mlp_ok(x, fc1, fc2):
        return "k23"
    if (C in (768, 1024) and x.numel() // C >= 1024
            and all(hot_ops.xs_linear_supported(x, w) for w in (qkv.weight, proj.weight, fc1.weight))):
        return "k24"
    return "k5"


def plan_stage(x, blk) -> StagePlan:
    """The plan of a stage whose blocks have `blk`'s layer shapes, for the token map x [B, D, H, W, C]."""
    flow = _stage_flow(x, blk)
    qkv, proj, fc1, fc2 = blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2
    hid = Stand(*x.shape[:-1], fc1.weight.shape[0], dtype=x.dtype, is_cuda=x.is_cuda)       # what fc2 reads
    if flow in ("k23", "k5"):           # already normalised input: each layer routes itself
        r_qkv = route_linear(x, qkv.weight, qkv.bias)
        if flow == "k23":
            return StagePlan(flow, r_qkv, route_linear(x, proj.weight, proj.bias, residual=x), "k23", None, None)
        return StagePlan(flow, r_qkv, route_linear(x, proj.weight, proj.bias), None,
                         route_linear(x, fc1.weight, fc1.bias, act="gelu"), "library")
    kernel = {"ws": "k13b", "k20": "k20", "k24": "k24"}[flow]
    if mlp_ok(x, fc1, fc2):             # C = 96 / 128 / 192, and 256 (Swin-B stage 1) under "k20"; never C = 768 / 1024
        return StagePlan(flow, kernel, kernel, "k23", None, None)
    if flow == "ws":                    # hidden width 4 C beyond K13 (f32 mode, C = 192 / 256): library GEMM + add
        r_fc2 = "k13b" if hot_ops.ws_linear_supported(hid, fc2.weight, False) else "library"
    else:                               # K20 or library + add (split_wins)
        r_fc2 = route_linear(hid, fc2.weight, fc2.bias, residual=x)
    return StagePlan(flow, kernel, kernel, None, kernel, r_fc2)
