"""Which kernel runs each pixel-sized linear layer of a forward, from the clip geometry alone.

The dispatch rules live in linear_routes.py (`route_linear`, `route_linear_multi`, `mlp_ok`, `plan_stage`); they only look at
shapes, dtypes, devices and the arithmetic mode, and the forward executes their answers (fused.linear, video_swin.BasicLayer).
This module asks them about the layers of a configuration with stand-in tensors and returns {call site: route}, so that

* `tests/test_routes.py` (CPU) pins the table of the BASELINE configurations (`tests/golden/routes.json`): a threshold that
  silently sends a layer back to the library GEMM fails a test instead of showing up as milliseconds;
* the same test on the GPU box checks that the launches a real forward records are the ones the table names.

    python -m neurips2023_soc_amd.routes --write      (re-generate the golden after a deliberate change)
"""
from __future__ import annotations

import json
import os
import sys
from types import SimpleNamespace
from typing import Dict

from . import hot_ops
from .linear_routes import Stand, mlp_ok, plan_stage, route_linear, route_linear_multi
from .video_swin import SWIN_CONFIGS

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "routes.json")
# BASELINE.json `configs`: Swin-T 360 x 640 (configs 0-2), Swin-B 720 x 1280 (3), Swin-B 360 x 640 (4); T = 8 throughout
BASELINE_GEOMETRIES = (("video-swin-t", 8, 360, 640), ("video-swin-b", 8, 720, 1280), ("video-swin-b", 8, 360, 640))
# a clip small enough that every stage stays below the row counts of the fused flows: all four stages take "k5"
SMALL_GEOMETRY = ("video-swin-t", 2, 128, 160)
D_MODEL, D_FFN = 256, 2048


def _lin(n: int, k: int, bias: bool = True):
    return SimpleNamespace(weight=Stand(n, k), bias=Stand(n) if bias else None)


def table(backbone: str, T: int, H: int, W: int, clips: int = 1) -> Dict[str, str]:
    """`clips` independent clips per launch group (the CLIPS of a graph_runner class): a batch of `clips`, so every
    pixel-sized layer sees `clips` times the rows."""
    cfg = SWIN_CONFIGS[backbone]
    T = T * clips                  # the routing predicates read row counts: frames of all clips of the group
    d = cfg["embed_dim"]
    h, w = -(-H // 4), -(-W // 4)
    out: Dict[str, str] = {}
    sizes = []
    for s in range(4):
        C = d * 2 ** s
        sizes.append((C, h, w))
        x = Stand(1, T, h, w, C)
        blk = SimpleNamespace(attn=SimpleNamespace(qkv=_lin(3 * C, C), proj=_lin(C, C)),
                              mlp=SimpleNamespace(fc1=_lin(4 * C, C), fc2=_lin(C, 4 * C)))
        plan = plan_stage(x, blk)
        out.update({f"swin{s}.{name}": route for name, route in plan._asdict().items() if route is not None})
        if s < 3:
            h, w = -(-h // 2), -(-w // 2)
            merged = Stand(1, T, h, w, 4 * C)
            out[f"merge{s}"] = route_linear(merged, Stand(2 * C, 4 * C), None)
    # input_proj of levels 1..3 (1x1 convolutions as GEMMs over tokens), fusion blocks, deformable encoder
    enc_rows = 0
    for lvl in (1, 2, 3):
        C, hh, ww = sizes[lvl]
        tok = Stand(T, hh * ww, C)
        out[f"input_proj{lvl}"] = route_linear(tok, Stand(D_MODEL, C), Stand(D_MODEL))
        seq = Stand(T * hh * ww, 1, D_MODEL)
        out[f"vlf{lvl}.q"] = route_linear(seq, Stand(D_MODEL, D_MODEL), Stand(D_MODEL), add=None)
        out[f"vlf{lvl}.out*tgt"] = route_linear(seq, Stand(D_MODEL, D_MODEL), Stand(D_MODEL), mul=seq)
        enc_rows += hh * ww
    _, hh, ww = sizes[3]
    enc_rows += -(-hh // 2) * -(-ww // 2)                  # the extra stride-64 level (3x3 stride-2 convolution: MIOpen)
    mem = Stand(T, enc_rows, D_MODEL)
    out["encoder.value_proj"] = route_linear(mem, Stand(D_MODEL, D_MODEL), Stand(D_MODEL))
    out["encoder.offsets|weights"] = route_linear_multi(
        mem, [(Stand(256, D_MODEL), Stand(256), True), (Stand(128, D_MODEL), Stand(128), True)], mem)
    out["encoder.output_proj"] = route_linear(mem, Stand(D_MODEL, D_MODEL), Stand(D_MODEL))
    out["encoder.ffn"] = "k23" if mlp_ok(mem, _lin(D_FFN, D_MODEL), _lin(D_MODEL, D_FFN)) else "library"
    return out


# what bench.py runs by default: groups of ten clips up to 360 x 640 (round 5: fours / eights), pairs above
HEADLINE_GROUP = ("video-swin-t", 8, 360, 640, 10)
GROUPED = (("video-swin-t", 8, 360, 640, 4), ("video-swin-b", 8, 360, 640, 4), ("video-swin-b", 8, 720, 1280, 2),
           ("video-swin-t", 8, 360, 640, 8), ("video-swin-b", 8, 360, 640, 8), HEADLINE_GROUP, ("video-swin-b", 8, 360, 640, 10))


def all_tables() -> Dict[str, Dict[str, str]]:
    tabs = {f"{b} T={t} {hh}x{ww}": table(b, t, hh, ww) for b, t, hh, ww in BASELINE_GEOMETRIES}
    tabs.update({f"{b} T={t} {hh}x{ww} x{c} clips": table(b, t, hh, ww, c) for b, t, hh, ww, c in GROUPED})
    with hot_ops.use_matmul_mode("f32"):
        tabs.update({f"{b} T={t} {hh}x{ww} f32": table(b, t, hh, ww) for b, t, hh, ww in BASELINE_GEOMETRIES})
        tabs.update({f"{b} T={t} {hh}x{ww} x{c} clips f32": table(b, t, hh, ww, c) for b, t, hh, ww, c in (HEADLINE_GROUP,)})
    tabs.update({f"{b} T={t} {hh}x{ww}": table(b, t, hh, ww) for b, t, hh, ww in (SMALL_GEOMETRY,)})
    return tabs


if __name__ == "__main__":
    tabs = all_tables()
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(tabs, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps(tabs, indent=1))
