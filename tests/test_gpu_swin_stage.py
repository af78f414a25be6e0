"""-m gpu: one Video-Swin stage (BasicLayer, two blocks so that a shifted one runs) at the smallest shape that takes each flow of
linear_routes.plan_stage, against the oracle's blocks chained in float64, with the launches it records checked against its plan."""
import functools

import pytest
import torch

from neurips2023_soc_amd import hot_ops, linear_routes
from neurips2023_soc_amd.video_swin import WINDOW, BasicLayer
from oracle import soc_oracle as O

# (flow, what the case is about, mode, width, token map [B, D, H, W]); 64 x 64 x 4 = 16 384 rows, 64 x 84 x 4 = 21 504
CASES = [
    ("ws", dict(mlp="k23"), "split", 96, (1, 4, 64, 64)),
    ("ws", dict(fc1="k13b", fc2="k13b"), "f32", 96, (1, 4, 64, 64)),
    ("ws", dict(fc1="k13b", fc2="library"), "f32", 192, (1, 4, 64, 64)),
    ("k20", dict(mlp="k23"), "split", 256, (1, 4, 64, 84)),
    ("k20", dict(fc1="k20"), "split", 1024, (1, 4, 64, 64)),
    ("k23", dict(mlp="k23"), "split", 384, (1, 4, 32, 32)),
    ("k24", dict(fc1="k24"), "split", 768, (1, 4, 16, 16)),
    ("k5", dict(fc2="library"), "split", 96, (1, 2, 14, 14)),
]
RECORDERS = {"k13b": hot_ops.record_ws_linear_calls, "k20": hot_ops.record_linear_split_calls,
             "k23": hot_ops.record_mlp_split_calls, "k24": hot_ops.record_xs_linear_calls}


def make_stage(C: int, dims, seed: int = 0):
    """(BasicLayer of width C with seeded, non-trivial parameters, its input [*dims, C]), both on the CPU."""
    torch.manual_seed(seed)
    layer = BasicLayer(C, 2, C // 32, WINDOW).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            if ".norm" in name:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith("relative_position_bias_table"):
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
    return layer, torch.randn(*dims, C, generator=g)


def oracle_chain(layer, x):
    """The oracle's blocks one after the other, in x's dtype on x's device."""
    sd = {k: v.detach().to(x) for k, v in layer.state_dict().items() if v.is_floating_point()}
    for i, blk in enumerate(layer.blocks):
        x = O.swin_block(sd, f"blocks.{i}", x, blk.attn.num_heads, blk.shift_size)
    return x


@functools.lru_cache(maxsize=None)
def reference(C: int, dims):
    """The float64 result on the CPU, computed once per (width, token map): two modes share the 96-wide one."""
    layer, x = make_stage(C, dims)
    with torch.no_grad():
        return oracle_chain(layer, x.double())


def recorded_shapes(calls, kernel):
    if kernel == "k23":
        return {(c["x"].numel() // c["w1"].shape[1], c["w1"].shape[1], c["w1"].shape[0]) for c in calls}
    return {(c["x"].numel() // c["weight"].shape[1], *c["weight"].shape) for c in calls}


@pytest.mark.gpu
@pytest.mark.parametrize("flow,named,mode,C,dims", CASES, ids=[f"{c[0]}-{c[2]}-{c[3]}" for c in CASES])
def test_stage_runs_its_plan_and_is_f32_grade(flow, named, mode, C, dims):
    """Error against float64 no larger than that of the same blocks in plain f32 torch ops on the device, with the margin of
    the f32-grade kernel tests (test_mlp_split_vs_f64: 1.5 x the f32 chain's error + 3e-7 of the output's scale); and each layer
    of a block is launched on the kernel its plan names, with its (rows, N, K), and on no other pixel kernel."""
    assert O.WINDOW == WINDOW
    layer, x = make_stage(C, dims)
    rows = x.numel() // C
    want = reference(C, dims)
    layer, xd = layer.cuda(), x.cuda()
    with hot_ops.use_matmul_mode(mode), torch.no_grad():
        plan = linear_routes.plan_stage(xd, layer.blocks[0])
        assert plan.flow == flow and all(getattr(plan, k) == v for k, v in named.items()), plan
        layer(xd)                                           # warm-up: weight images, caches
        for rec in RECORDERS.values():
            rec(True)
        got = layer(xd)
        seen = {kernel: recorded_shapes(rec(False), kernel) for kernel, rec in RECORDERS.items()}
    with torch.device("cuda"), torch.no_grad():             # the oracle's factory calls (masks, indices) on the device
        plain = oracle_chain(layer, xd)
    shapes = {"qkv": (rows, 3 * C, C), "proj": (rows, C, C), "mlp": (rows, C, 4 * C), "fc1": (rows, 4 * C, C), "fc2": (rows, C, 4 * C)}
    planned = {kernel: {shapes[k] for k, v in plan._asdict().items() if v == kernel and k != "flow"} for kernel in RECORDERS}
    assert seen == planned, (plan, seen)
    scale = float(want.abs().max())
    e_ours, e_f32 = float((got.cpu().double() - want).abs().max()), float((plain.cpu().double() - want).abs().max())
    print(f"stage {flow} {mode} C={C}: ours {e_ours / scale:.2e}  plain f32 {e_f32 / scale:.2e}  ratio {e_ours / e_f32:.2f}")
    assert e_ours <= 1.5 * e_f32 + 3e-7 * scale, (e_ours, e_f32, scale)
