"""Linear layers of the hot path, launched on the kernel that linear_routes.py names: `linear` runs
mul * act(LN(x [+ add]) @ W.T + b) + residual on K7 (few rows: queries, words), K12, K13 / K13b, K20, K24 or the library GEMM
(hipBLASLt / rocBLAS through torch, kernel chosen by gemm_tuning's table, ReLU in its epilogue), `linear_multi` several layers on
one input, `ffn_relu` a two-layer block (K23 where it covers the shape).  A caller that holds a plan passes `route=`."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import hot_ops
from .linear_routes import is_small, mlp_ok, route_linear, route_linear_multi  # noqa: F401  (callers and tests use fused.<name>)


def ffn_relu(x: torch.Tensor, lin1: nn.Linear, lin2: nn.Linear) -> torch.Tensor:
    """lin2(relu(lin1(x))) -- the deformable encoder's feed-forward block (reference models/deformable_transformer.py:
    253-263): K23 in one launch where it covers the shape (the encoder layer calls it with the residual and norm2 folded in as
    well), the two-GEMM path otherwise (SOC_MATMUL=f32, SOC_SPLIT_OFF=mlp, few rows)."""
    if mlp_ok(x, lin1, lin2):
        return hot_ops.mlp_split(x, lin1.weight, lin1.bias, lin2.weight, lin2.bias, "relu")
    return apply(lin2, linear_relu(x, lin1))


def _cannot(route: str, **args) -> None:
    if any(v is not None for v in args.values()):
        raise ValueError(f"fused.linear: route {route!r} cannot take {[k for k, v in args.items() if v is not None]}")


def _behind(y, mul, residual):
    if mul is not None:
        y = y * mul
    return y if residual is None else y + residual


def _k7(x, weight, bias, ln, residual, act, add, mul):
    _cannot("k7", ln=ln, gelu=act if act == "gelu" else None)
    if add is not None and add.shape != x.shape:
        add = add.expand_as(x)
    return _behind(hot_ops.linear_small(x, weight, bias, add, act == "relu"), mul, residual)


def _k12(x, weight, bias, ln, residual, act, add, mul):
    _cannot("k12", ln=ln, residual=residual, add=add, mul=mul)
    return hot_ops.linear_act(x, weight, bias, act)


def _k13b(x, weight, bias, ln, residual, act, add, mul):
    _cannot("k13b", add=add, mul=mul)
    return hot_ops.ws_linear(x, weight, bias, ln, residual, act)


def _k24(x, weight, bias, ln, residual, act, add, mul):
    _cannot("k24", add=add, mul=mul)
    return hot_ops.xs_linear(x, weight, bias, ln, residual, act)


def _library(x, weight, bias, ln, residual, act, add, mul):
    _cannot("library", ln=ln)
    if add is not None:
        x = x + add
    if act == "relu" and bias is not None:          # the ReLU in the GEMM's epilogue (hipBLASLt RELU_BIAS)
        y = torch._addmm_activation(bias, x.reshape(-1, x.shape[-1]), weight.t(), use_gelu=False)
        y = y.view(*x.shape[:-1], y.shape[-1])
    else:
        y = F.linear(x, weight, bias)
        y = F.relu(y) if act == "relu" else F.gelu(y) if act == "gelu" else y
    return _behind(y, mul, residual)                # a pass for each


def _k20(x, weight, bias, ln, residual, act, add, mul):       # every part of the expression is part of the launch
    return hot_ops.linear_split(x, weight, bias, ln, residual, act, add, mul)


_LAUNCH = {"k7": _k7, "k12": _k12, "k13b": _k13b, "k20": _k20, "k24": _k24, "library": _library}


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
           add: Optional[torch.Tensor] = None, relu: bool = False, mul: Optional[torch.Tensor] = None,
           residual: Optional[torch.Tensor] = None, *, ln: Optional[Tuple[torch.Tensor, torch.Tensor, float]] = None,
           act: str = "none", route: Optional[str] = None) -> torch.Tensor:
    """mul * act(LN(x [+ add]) @ weight.T + bias) + residual; `add` broadcasts like `x + add`, ln = (gamma, beta, eps), act is
    "none" | "relu" | "gelu" (exact, erf), `relu=True` spells act="relu".  Runs on `route` (a label of linear_routes) and on nothing
    else where the caller holds a plan, on the kernel route_linear names otherwise; a route that cannot take an argument raises."""
    if relu:
        act = "relu"
    if route is None:
        route = route_linear(x, weight, bias, ln=ln is not None, add=add, act=act, mul=mul, residual=residual)
        if route == "library" and (mul is not None or residual is not None):
            # no kernel takes the whole expression: the layer itself wherever it goes without them, then a pass for each
            return _behind(linear(x, weight, bias, add, ln=ln, act=act), mul, residual)
    return _LAUNCH[route](x, weight, bias, ln, residual, act, add, mul)


def linear_multi(x: torch.Tensor, layers, add: Optional[torch.Tensor] = None):
    """[(x + add if use_add else x) @ W.T + b for (W, b, use_add) in layers] on the kernel route_linear_multi names."""
    route = route_linear_multi(x, layers, add)
    if route == "k7":
        return hot_ops.linear_small_multi(x, layers, add)
    if route == "k20":
        # K20 with two outputs: both layers' rows stacked into one weight image (cached), x + pos in the loader
        w, b = _stacked(layers[0][0], layers[0][1], layers[1][0], layers[1][1])
        return list(hot_ops.linear_split(x, w, b, add=add, split_at=layers[0][0].shape[0]))
    if route == "k12":
        # two pixel-sized layers on x + pos (the deformable encoder's sampling offsets and attention weights):
        # one K12 launch with the add in its prologue instead of an add kernel and two library GEMMs
        return hot_ops.linear_act_multi(x, [(w, b) for w, b, _ in layers], add)
    xa = x + add if (add is not None and any(u for _, _, u in layers)) else x
    return [F.linear(xa if u else x, w, b) for w, b, u in layers]


_stack_cache = hot_ops.DerivedCache()


def _stacked(w0, b0, w1, b1):
    """cat of two layers' (weight, bias), cached until one of them changes (K20 packs the stacked matrix once) and freed
    with the layers."""
    return _stack_cache.get((w0, b0, w1, b1), lambda: (torch.cat([w0.detach(), w1.detach()], 0).contiguous(),
                                                      torch.cat([b0.detach(), b1.detach()], 0).contiguous()))


def linear_relu(x: torch.Tensor, lin: nn.Linear) -> torch.Tensor:
    """relu(x @ W^T + b).  Many rows: the ReLU runs in the GEMM epilogue, bit-identical to F.relu(lin(x)) and one read+write
    pass over the activation less (316 MB per deformable-encoder FFN at the BASELINE config).  Few rows: K7."""
    return linear(x, lin.weight, lin.bias, act="relu")


def linear_gelu(x: torch.Tensor, lin: nn.Linear) -> torch.Tensor:
    """gelu(lin(x)), exact (erf) GELU: K24 / K13b / K20 / K12 apply it to the accumulators; elsewhere the library GEMM + a GELU pass."""
    return linear(x, lin.weight, lin.bias, act="gelu")


def apply(lin: nn.Linear, x: torch.Tensor, add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lin(x [+ add]) through `linear`."""
    return linear(x, lin.weight, lin.bias, add=add)
