"""-m gpu: the memory contract of every kernel entry point (include/soc_hip.h: "inputs are borrowed, outputs are
caller-allocated and fully overwritten"), checked with guarded allocations (tests/guarded.py) at tile-edge shapes.

One table (CASES): the C entry point a case claims, a builder of CPU inputs, the hot_ops call, an f64 reference and the
tolerance of that kernel's existing test in tests/test_gpu_kernels.py (tests/test_clip_io.py, tests/test_gpu_davis_eval.py for
K6 / K9 / K27) -- no tolerance is introduced here.  Every case runs twice on identical inputs, once per guard pattern:
  1 every guard byte of every input, output, workspace and packed weight image is intact;
  2 the outputs of the two runs are bit-identical (nothing left unwritten, nothing depends on prior memory contents);
  3 every input is bit-identical before and after (except the documented in-place operand);
  4 run 1 agrees with the f64 reference;     5 the claimed soc_* entry point was reached.
Then: the header's six aliasing clauses, and row isolation of the ten row-wise kernels under NaN / +Inf rows.
tests/test_guarded_helper.py (CPU) proves that the checks bite and that every kernel entry point is claimed here."""
from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import soc_oracle as O
from tests import guarded as G

pytestmark = pytest.mark.gpu

D64 = torch.float64
ROWS = ("1", "t-1", "t", "t+1", "2t+1")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from neurips2023_soc_amd import hot_ops
    return hot_ops


def rows_of(sym: str, t: int) -> int:
    return {"1": 1, "t-1": max(t - 1, 1), "t": t, "t+1": t + 1, "2t+1": 2 * t + 1}[sym]


def gen(*key) -> torch.Generator:
    """A generator seeded by the case's parameters (no str hashing: the seed must not change between processes)."""
    return torch.Generator().manual_seed(sum((i + 1) * sum(ord(c) for c in str(k)) for i, k in enumerate(key)))


def rn(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g) * scale + shift


def act_of(y, act):
    return F.gelu(y) if act == "gelu" else (y.relu() if act == "relu" else y)


def d(t):
    return None if t is None else t.double()


def absmax(w):
    return float(w.abs().max()) if w.numel() else 0.0


def rel(k):
    """k * max(1, |want|max): the form of most bounds in tests/test_gpu_kernels.py."""
    return lambda i, w: k * max(1.0, absmax(w))


def scale_of(k):
    """k * |want|max (K23 / K24)."""
    return lambda i, w: k * absmax(w)


def fixed(*ks):
    """Absolute bounds, one per output (the last repeats); 0 = bit-exact."""
    return lambda i, w: ks[min(i, len(ks) - 1)]


@dataclass
class Built:
    inputs: dict
    call: Callable                        # (ops, tensors on the device) -> tensor | tuple
    ref: Callable                         # (CPU inputs) -> f64 tensor | tuple
    tol: Optional[Callable] = None        # (output index, want) -> bound
    inplace: Sequence[str] = ()
    compare: Optional[Callable] = None    # (output index, got, want): custom judgement instead of tol


@dataclass
class Case:
    id: str
    entry: str
    make: Callable                        # (ops) -> Built
    also: Tuple[str, ...] = ()            # further entry points the call must reach (pack kernels, row statistics)


CASES = []


def case(id, entry, make, also=()):
    CASES.append(Case(id, entry, make, tuple(also)))


# ------------------------------------------------------------------------------------------------- K2 MSDA
_LEVELS = torch.tensor([[7, 5], [5, 3], [3, 2], [1, 1]])
_LEVELS_P2 = torch.tensor([[8, 4], [4, 2], [2, 2], [1, 1]])


def _lsi(shapes):
    return torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))


def _msda_fwd(N, Lq, M, Dh, dt):
    def make(ops):
        g = gen("msda", N, Lq, M, Dh)
        S, L, P = int(_LEVELS.prod(1).sum()), 4, 4
        inp = dict(value=rn(g, N, S, M, Dh).to(dt), shapes=_LEVELS.clone(), lsi=_lsi(_LEVELS),
                   loc=(torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.3 - 0.15).to(dt),
                   w=torch.softmax(rn(g, N, Lq, M, L * P), -1).view(N, Lq, M, L, P).to(dt))
        return Built(inp, lambda ops, t: ops.msda_forward(t["value"], t["shapes"], t["lsi"], t["loc"], t["w"]),
                     lambda t: O.msda_core(d(t["value"]), t["shapes"], t["lsi"], d(t["loc"]), d(t["w"])),
                     fixed(3e-5 if dt == torch.float32 else 1e-12))
    return make


for N, Lq in ((1, 1), (1, 77), (3, 301)):
    case(f"msda_fwd_f32-N{N}-Lq{Lq}", "soc_msda_fwd_f32", _msda_fwd(N, Lq, 8, 32, torch.float32))
case("msda_fwd_f32-D16", "soc_msda_fwd_f32", _msda_fwd(2, 5, 8, 16, torch.float32))
case("msda_fwd_f64-N1", "soc_msda_fwd_f64", _msda_fwd(1, 7, 2, 16, torch.float64))
case("msda_fwd_f64-N3", "soc_msda_fwd_f64", _msda_fwd(3, 33, 8, 32, torch.float64))


def _msda_bwd(N, Lq, M, Dh, dt):
    """grad_value is accumulated with atomics (the entry point zeroes it with hipMemsetAsync first), so the order of the
    additions is not fixed.  Check 2 stays: every operand here is a short dyadic rational (power-of-two level sizes,
    sampling points on a 1/32 grid, weights and gradients on 1/8 grids), so every product and every partial sum is exact in
    f32 and the result cannot depend on the order."""
    def make(ops):
        g = gen("msda_bwd", N, Lq, M, Dh)
        S, L, P = int(_LEVELS_P2.prod(1).sum()), 4, 4

        def grid(*shape, lo, hi, step):
            return (torch.randint(lo, hi + 1, shape, generator=g).double() * step).to(dt)
        inp = dict(value=grid(N, S, M, Dh, lo=-8, hi=8, step=0.125), shapes=_LEVELS_P2.clone(), lsi=_lsi(_LEVELS_P2),
                   loc=grid(N, Lq, M, L, P, 2, lo=-8, hi=40, step=1 / 32), w=grid(N, Lq, M, L, P, lo=0, hi=8, step=0.125),
                   go=grid(N, Lq, M * Dh, lo=-8, hi=8, step=0.125))
        k = 2e-5 if dt == torch.float32 else 1e-11
        return Built(inp, lambda ops, t: ops.msda_backward(t["value"], t["shapes"], t["lsi"], t["loc"], t["w"], t["go"]),
                     lambda t: O.msda_backward_core(d(t["value"]), t["shapes"], t["lsi"], d(t["loc"]), d(t["w"]), d(t["go"])),
                     rel(k))
    return make


case("msda_bwd_f32-N2", "soc_msda_bwd_f32", _msda_bwd(2, 50, 8, 32, torch.float32))
case("msda_bwd_f32-N1-D64", "soc_msda_bwd_f32", _msda_bwd(1, 9, 4, 64, torch.float32))
case("msda_bwd_f64-D71", "soc_msda_bwd_f64", _msda_bwd(1, 7, 2, 71, torch.float64))
case("msda_bwd_f64-N3", "soc_msda_bwd_f64", _msda_bwd(3, 9, 4, 16, torch.float64))


def _msda_fused(N, Lq, rd, padding):
    def make(ops):
        g = gen("fused", N, Lq, rd)
        S, M = int(_LEVELS.prod(1).sum()), 8
        ref = torch.rand(N, Lq, 4, rd, generator=g)
        if rd == 4:
            ref[..., 2:] *= 0.5
        inp = dict(value=rn(g, N, S, M, 32), shapes=_LEVELS.clone(), lsi=_lsi(_LEVELS), ref=ref,
                   off=rn(g, N, Lq, M, 4, 4, 2, scale=3.0), logits=rn(g, N, Lq, M, 16))
        if padding:
            inp["pad"] = torch.rand(N, S, generator=g) < 0.3
            inp["flag"] = inp["pad"].any().to(torch.int32).reshape(1)
        return Built(inp, lambda ops, t: ops.msda_fused_forward(t["value"], t["shapes"], t["lsi"], t["ref"], t["off"], t["logits"],
                                                                t.get("pad"), t.get("flag")),
                     lambda t: O.msda_fused_core(d(t["value"]), t["shapes"], t["lsi"], d(t["ref"]), d(t["off"]), d(t["logits"]),
                                                 t.get("pad")), fixed(3e-5))
    return make


for N, Lq, rd, pad in ((1, 1, 2, False), (3, 77, 2, True), (2, 20, 4, True), (1, 301, 4, False)):
    case(f"msda_fused-N{N}-Lq{Lq}-rd{rd}-pad{int(pad)}", "soc_msda_fused_fwd_f32", _msda_fused(N, Lq, rd, pad))


# ------------------------------------------------------------------------------------------------- K1 window attention
def _win(B, Dd, H, W, nH, shift):
    def make(ops):
        g = gen("win", B, Dd, H, W, nH)
        Cc = nH * 32
        inp = dict(qkv=rn(g, B, Dd, H, W, 3 * Cc), bias=rn(g, 3 * Cc, scale=0.5), table=rn(g, 15 * 13 * 13, nH, scale=0.5))
        return Built(inp, lambda ops, t: ops.window_attention3d(t["qkv"], t["bias"], t["table"], nH, O.WINDOW, shift),
                     lambda t: O.window_attention_core(d(t["qkv"]), d(t["bias"]), d(t["table"]), nH, O.WINDOW, shift), rel(2e-5))
    return make


for B, Dd, H, W, nH, shift in ((1, 8, 14, 21, 3, (0, 0, 0)), (1, 8, 14, 21, 3, (4, 3, 3)),      # full 8x7x7 windows: the split form
                               (1, 1, 7, 11, 1, (0, 0, 0)), (1, 3, 11, 13, 2, (4, 3, 3)),      # T = 1; prime H and W, padded windows
                               (2, 10, 5, 7, 1, (4, 3, 3))):                                   # temporal shift, D padded to 16
    case(f"win_attn3d-B{B}-{Dd}x{H}x{W}-h{nH}-s{shift[0]}", "soc_win_attn3d_f32", _win(B, Dd, H, W, nH, shift))


# ------------------------------------------------------------------------------------------------- K3 attention core
def _mha(Lq, Lk, B, pad, batch_first, masked):
    def make(ops):
        g = gen("mha", Lq, Lk, B, pad, batch_first, masked)
        shp = (lambda n: (B, n, 256)) if batch_first else (lambda n: (n, B, 256))
        inp = dict(q=rn(g, *shp(Lq)), k=rn(g, *shp(Lk)), v=rn(g, *shp(Lk)))
        if pad:
            inp["kpm"] = torch.zeros(B, Lk, dtype=torch.bool)
            inp["kpm"][:, Lk - pad:] = True
        if masked:
            m = torch.where(torch.rand(B * masked, Lq, Lk, generator=g) < 0.3, -1000.0, 0.0)
            m[:, :, 0] = 0.0
            inp["mask"] = m
        return Built(inp, lambda ops, t: ops.mha_core(t["q"], t["k"], t["v"], 8, t.get("kpm"), batch_first, t.get("mask")),
                     lambda t: O.mha_core(d(t["q"]), d(t["k"]), d(t["v"]), 8, t.get("kpm"), batch_first, d(t.get("mask"))),
                     fixed(2e-5))
    return make


for Lq, Lk, B, pad, bf, masked in ((1, 1, 1, 0, False, 0), (13, 7, 1, 2, False, 0), (67, 131, 2, 0, False, 0), (61, 13, 3, 4, True, 0),
                                   (17, 257, 1, 0, True, 0), (31, 29, 2, 0, False, 1), (31, 29, 2, 0, False, 8)):
    case(f"xattn-{Lq}x{Lk}-B{B}-pad{pad}-bf{int(bf)}-m{masked}", "soc_xattn_f32", _mha(Lq, Lk, B, pad, bf, masked))


# ------------------------------------------------------------------------------------------------- K4 dynamic mask head
def _dyn(T, Q, h, w):
    def make(ops):
        g = gen("dyn", T, Q, h, w)
        inp = dict(feats=rn(g, T, 8, h, w), params=rn(g, T * Q, 169, scale=0.2), refs=torch.rand(T * Q, 2, generator=g))
        return Built(inp, lambda ops, t: ops.dynamic_mask(t["feats"], t["params"], t["refs"], (4 * h, 4 * w)),
                     lambda t: O.dynamic_mask_core(d(t["feats"]), d(t["params"]), d(t["refs"]), (4 * h, 4 * w)), rel(1e-5))
    return make


for T, Q, h, w in ((1, 1, 3, 5), (2, 7, 31, 17), (1, 20, 13, 67)):
    case(f"dyn_mask-T{T}-Q{Q}-{h}x{w}", "soc_dyn_mask_f32", _dyn(T, Q, h, w))


# ------------------------------------------------------------------------------------------------- K5 add + LayerNorm
def aln_tile(Cc):
    """Rows per workgroup iteration, csrc/add_layernorm.hip: RPB = 4 * (64 / G) * UNR of the instance taken for C."""
    nvec = Cc // 4
    g, unr = (32, 4) if nvec <= 32 else (64, 4) if nvec <= 64 else (64, 2) if nvec <= 192 else (64, 1)
    return 4 * (64 // g) * unr


def _aln(sym, Cc, with_y, return_sum=True):
    def make(ops):
        rows = rows_of(sym, aln_tile(Cc))
        g = gen("aln", rows, Cc)
        inp = dict(x=rn(g, rows, Cc, scale=3.0, shift=1.0), w=rn(g, Cc), b=rn(g, Cc))
        if with_y:
            inp["y"] = rn(g, rows, Cc)

        def ref(t):
            s, n = O.add_layernorm_core(d(t["x"]), d(t.get("y")), d(t["w"]), d(t["b"]), 1e-5)
            return (s if with_y and return_sum else None), n
        return Built(inp, lambda ops, t: tuple(o if (o is not t["x"]) else None for o in
                                               ops.add_layernorm(t["x"], t.get("y"), t["w"], t["b"], 1e-5, return_sum=return_sum)),
                     ref, fixed(0.0, 2e-5))         # the sum is one f32 add: bit-exact against the rounded f64 sum
    return make


for Cc in (96, 256, 768, 2048):
    for sym in ROWS:
        case(f"add_layernorm-C{Cc}-rows_{sym}", "soc_add_layernorm_f32", _aln(sym, Cc, True))
case("add_layernorm-C4-plain", "soc_add_layernorm_f32", _aln("t+1", 4, False))
case("add_layernorm-C1536-plain", "soc_add_layernorm_f32", _aln("2t+1", 1536, False))
case("add_layernorm-C96-nosum", "soc_add_layernorm_f32", _aln("t+1", 96, True, return_sum=False))


# ------------------------------------------------------------------------------------------------- K6 up-sampling forms
def _upthr(T, h, w, H0, W0):
    def make(ops):
        g = gen("upthr", T, h, w, H0, W0)
        inp = dict(x=rn(g, T, h, w, scale=5.0))

        def compare(i, got, up):
            diff = got != (up > 0)
            assert int(diff.sum()) <= max(2, diff.numel() // 200000), int(diff.sum())
            if diff.any():          # identical except where the up-sampled logit is within 1e-5 of the threshold
                assert float(up[diff].abs().max()) < 1e-5, float(up[diff].abs().max())
        return Built(inp, lambda ops, t: ops.upsample_threshold(t["x"], (H0, W0)),
                     lambda t: F.interpolate(d(t["x"])[None], size=(H0, W0), mode="bilinear", align_corners=False)[0],
                     compare=compare)
    return make


for T, h, w, H0, W0 in ((1, 5, 7, 33, 50), (3, 7, 11, 29, 37), (1, 9, 9, 9, 9), (2, 13, 17, 53, 127), (1, 3, 3, 5, 15)):
    case(f"upsample_threshold-T{T}-{h}x{w}-to-{H0}x{W0}", "soc_upsample_threshold_u8", _upthr(T, h, w, H0, W0))


def _upmerge(Ob, T, h, w, H0, W0):
    def make(ops):
        g = gen("upmerge", Ob, T, h, w, H0, W0)
        logits = rn(g, Ob, T, h, w, scale=4.0)
        # saturated sigmoids: exact ties between objects.  +40 keeps every up-sampled logit of that half above 17, where the f32
        # sigmoid is exactly 1: between 14 and 17 it is 1 - a few ulps, and which object wins there is rounding noise of exp
        logits[:, :, : h // 2] += 40.0

        def scores(t):
            up = F.interpolate(d(t["x"]), size=(H0, W0), mode="bilinear", align_corners=False).sigmoid()
            m = up.clone()
            m[m < 0.5] = 0.0
            # the scores are f32 values by definition (saturated sigmoids are exactly 1 and tie): f64 arithmetic, rounded once
            return up.float(), torch.cat([torch.full((1, T, H0, W0), 0.1, dtype=D64), m], 0).float()

        def compare(i, got, want_scores):
            up, sc = want_scores
            bad = got.long() != sc.argmax(0)
            if bad.any():           # only where the two best scores are closer than the fp32 noise of interpolate + exp
                top2 = sc.topk(2, 0)[0]
                assert float((top2[0] - top2[1])[bad].max()) < 1e-6 or float((up - 0.5).abs().min(0)[0][bad].max()) < 1e-6
            assert float(bad.float().mean()) < 1e-4
        return Built(dict(x=logits), lambda ops, t: ops.upsample_merge_labels(t["x"], (H0, W0)), lambda t: (scores(t),),
                     compare=compare)
    return make


for Ob, T, h, w, H0, W0 in ((1, 2, 9, 11, 31, 50), (3, 1, 7, 5, 23, 37), (5, 1, 13, 11, 13, 11)):
    case(f"upsample_merge_labels-O{Ob}-T{T}-{h}x{w}-to-{H0}x{W0}", "soc_upsample_merge_labels_u8", _upmerge(Ob, T, h, w, H0, W0))


# ------------------------------------------------------------------------------------------------- K9 resize + normalise
def _resize(T, H0, W0, h, w):
    def make(ops):
        from neurips2023_soc_amd import clip_io as CI
        from oracle import resize_oracle as R
        rng = np.random.default_rng(H0 * W0 + h)
        frames = rng.integers(0, 256, (T, H0, W0, 3)).astype(np.uint8)
        (bx, kx), (by, ky) = CI.resample_tables(W0, w), CI.resample_tables(H0, h)
        inp = dict(frames=torch.from_numpy(frames), bx=torch.from_numpy(bx), kx=torch.from_numpy(kx), by=torch.from_numpy(by),
                   ky=torch.from_numpy(ky))

        def ref(t):
            small = np.stack([R.resize_bilinear_u8(f, h, w) for f in t["frames"].numpy()])
            x = small.astype(np.float32) / np.float32(255)
            x = (x - np.asarray(CI.IMAGENET_MEAN, dtype=np.float32)) / np.asarray(CI.IMAGENET_STD, dtype=np.float32)
            return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))), torch.from_numpy(small)
        return Built(inp, lambda ops, t: ops.resize_normalize(t["frames"], (h, w), (t["bx"], t["kx"]), (t["by"], t["ky"]),
                                                              CI.IMAGENET_MEAN, CI.IMAGENET_STD, return_u8=True),
                     ref, fixed(0.0))          # PIL's bytes and the same fp32 bits (tests/test_clip_io.py)
    return make


for T, H0, W0, h, w in ((1, 37, 53, 19, 23), (2, 41, 29, 31, 37), (1, 17, 97, 17, 41), (3, 13, 11, 29, 11)):
    case(f"resize_normalize-T{T}-{H0}x{W0}-to-{h}x{w}", "soc_resize_normalize_u8_f32", _resize(T, H0, W0, h, w))


# ------------------------------------------------------------------------------------------------- K7 small-M linear
def _lin_small(sym, N, K, add, relu, bias, direct=False):
    def make(ops):
        M = rows_of(sym, 16)                               # one MFMA row tile (csrc/linear_small.hip)
        g = gen("lsmall", M, N, K, add)
        inp = dict(x=rn(g, M, K), w=rn(g, N, K, scale=K ** -0.5))
        if bias:
            inp["b"] = rn(g, N)
        if add:
            inp["a"] = rn(g, M, K)

        def call(ops, t):
            if not direct:
                return ops.linear_small(t["x"], t["w"], t.get("b"), t.get("a"), relu)
            from neurips2023_soc_amd import _lib
            out = torch.empty(M, N, dtype=torch.float32, device=t["x"].device)
            ptr = lambda v: None if v is None else v.data_ptr()      # noqa: E731
            _lib.check(_lib.load().soc_linear_small_f32(ptr(t["x"]), ptr(t.get("a")), 1, M, ptr(t["w"]), ptr(t.get("b")), ptr(out),
                                                        M, N, K, int(relu), ops._stream()), "soc_linear_small_f32")
            return out
        return Built(inp, call, lambda t: O.linear_core(d(t["x"]), d(t["w"]), d(t.get("b")), d(t.get("a")), relu), rel(2e-5))
    return make


for N, K, add, relu, bias in ((256, 256, False, False, True), (169, 256, True, False, True), (2, 256, False, False, True),
                              (40, 48, True, True, True), (768, 3072, False, False, False)):
    for sym in ROWS:
        case(f"linear_small-N{N}-K{K}-rows_{sym}", "soc_linear_small_multi_f32", _lin_small(sym, N, K, add, relu, bias))
for sym in ROWS:
    case(f"linear_small_single-rows_{sym}", "soc_linear_small_f32", _lin_small(sym, 169, 48, True, True, True, direct=True))


def _lin_small_multi(sym):
    def make(ops):
        M = rows_of(sym, 16)
        g = gen("lsmulti", M)
        ns, use = (256, 132, 40, 2), (True, True, False, True)
        inp = dict(x=rn(g, M, 256), a=rn(g, M, 256))
        for i, n in enumerate(ns):
            inp[f"w{i}"] = rn(g, n, 256, scale=1 / 16)
            if i != 3:
                inp[f"b{i}"] = rn(g, n)
        return Built(inp, lambda ops, t: tuple(ops.linear_small_multi(t["x"], [(t[f"w{i}"], t.get(f"b{i}"), use[i]) for i in range(4)],
                                                                      t["a"])),
                     lambda t: tuple(O.linear_core(d(t["x"]), d(t[f"w{i}"]), d(t.get(f"b{i}")), d(t["a"]) if use[i] else None)
                                     for i in range(4)), rel(2e-5))
    return make


for sym in ROWS:
    case(f"linear_small_multi-rows_{sym}", "soc_linear_small_multi_f32", _lin_small_multi(sym))


# ------------------------------------------------------------------------------------------------- K8 box refinement
def _box(N, Q, L, rd, with_vr):
    def make(ops):
        g = gen("box", N, Q, rd)
        ref = torch.rand(N, Q, rd, generator=g)
        ref[0, 0, 0] = 0.0
        inp = dict(delta=rn(g, N, Q, 4, scale=2.0), ref=ref)
        if with_vr:
            inp["vr"] = torch.rand(N, L, 2, generator=g) * 0.5 + 0.5
        return Built(inp, lambda ops, t: ops.box_refine(t["delta"], t["ref"], t.get("vr")),
                     lambda t: O.box_refine_core(d(t["delta"]), d(t["ref"]), d(t.get("vr"))), fixed(1e-6))
    return make


for N, Q, rd, vr in ((1, 1, 2, True), (3, 7, 4, True), (8, 20, 2, False), (5, 67, 4, True)):
    case(f"box_refine-N{N}-Q{Q}-rd{rd}-vr{int(vr)}", "soc_box_refine_f32", _box(N, Q, 4, rd, vr))


# ------------------------------------------------------------------------------------------------- K10 GroupNorm on tokens
def gn_tile(Cc):
    """Rows of S per workgroup, csrc/groupnorm_tokens.hip rows_per_block()."""
    return 64 * max(1, 256 // Cc)


def _gn_tok(N, sym, Cc, Gr, shift, relu):
    def make(ops):
        S = rows_of(sym, gn_tile(Cc))
        g = gen("gntok", N, S, Cc)
        inp = dict(x=rn(g, N, S, Cc, scale=2.0, shift=shift), w=rn(g, Cc), b=rn(g, Cc))

        def ref(t):
            y = O.groupnorm_tokens_core(d(t["x"]), d(t["w"]), d(t["b"]), Gr, 1e-5)
            return y.relu() if relu else y
        return Built(inp, lambda ops, t: ops.groupnorm_tokens(t["x"], t["w"], t["b"], Gr, 1e-5, relu=relu), ref, rel(3e-5))
    return make


for N, Cc, Gr, shift, relu in ((1, 256, 32, 0.0, False), (3, 256, 8, 50.0, True), (2, 16, 8, 3.0, True), (3, 64, 8, -7.0, False)):
    for sym in ROWS:
        case(f"groupnorm_tokens-N{N}-C{Cc}-G{Gr}-S_{sym}", "soc_groupnorm_tokens_f32", _gn_tok(N, sym, Cc, Gr, shift, relu))


# ------------------------------------------------------------------------------------------------- K11 / K21 Video-Swin edges
def _pmerge(B, Dd, H, W, Cc):
    def make(ops):
        g = gen("pmerge", B, Dd, H, W, Cc)
        inp = dict(x=rn(g, B, Dd, H, W, Cc, scale=2.0, shift=0.5), w=rn(g, 4 * Cc), b=rn(g, 4 * Cc))
        return Built(inp, lambda ops, t: ops.patch_merge_layernorm(t["x"], t["w"], t["b"], 1e-5),
                     lambda t: O.patch_merge_layernorm_core(d(t["x"]), d(t["w"]), d(t["b"]), 1e-5), fixed(3e-5))
    return make


# one wave per output row, four per workgroup (csrc/patch_merge.hip): output rows 1, 3, 4, 5, 9 and prime H, W
for B, Dd, H, W, Cc in ((1, 1, 1, 1, 512), (1, 1, 2, 5, 96), (1, 1, 4, 4, 96), (1, 1, 2, 9, 128), (1, 1, 5, 5, 192),
                        (2, 3, 7, 5, 128), (1, 2, 11, 13, 384)):
    case(f"patch_merge-{B}x{Dd}x{H}x{W}-C{Cc}", "soc_patch_merge_layernorm_f32", _pmerge(B, Dd, H, W, Cc))


def _pembed(N, H, W, Cc, bias):
    def make(ops):
        g = gen("pembed", N, H, W, Cc)
        inp = dict(frames=rn(g, N, 3, H, W), w=rn(g, Cc, 3, 1, 4, 4, scale=0.2), gam=torch.rand(Cc, generator=g) + 0.5,
                   bet=rn(g, Cc, scale=0.1))
        if bias:
            inp["b"] = rn(g, Cc, scale=0.1)

        def ref(t):
            x = F.pad(d(t["frames"]), (0, -W % 4, 0, -H % 4))
            y = F.conv2d(x, d(t["w"])[:, :, 0], d(t.get("b")), stride=4).permute(0, 2, 3, 1)
            return F.layer_norm(y, (Cc,), d(t["gam"]), d(t["bet"]), 1e-5)
        return Built(inp, lambda ops, t: ops.patch_embed_layernorm(t["frames"], t["w"], t.get("b"), t["gam"], t["bet"], 1e-5), ref,
                     fixed(2e-5))
    return make


# 64 tokens per tile (csrc/patch_embed.hip TOK): 1, 63, 64, 65 and 129+ tokens, ragged right / bottom edges
for N, H, W, Cc, bias in ((1, 4, 4, 96, True), (1, 28, 36, 96, True), (1, 32, 32, 128, True), (1, 20, 52, 96, False),
                          (1, 43, 47, 128, True), (3, 17, 23, 96, True)):
    case(f"patch_embed-N{N}-{H}x{W}-C{Cc}-b{int(bias)}", "soc_patch_embed_layernorm_f32", _pembed(N, H, W, Cc, bias))


# ------------------------------------------------------------------------------------------------- K12 tiled GEMM + activation
def _lin_act(sym, N, K, act, bias):
    def make(ops):
        M = rows_of(sym, 128)                              # BM = 128 (csrc/linear_tiled.hip)
        g = gen("lact", M, N, K)
        inp = dict(x=rn(g, M, K), w=rn(g, N, K, scale=K ** -0.5))
        if bias:
            inp["b"] = rn(g, N)
        return Built(inp, lambda ops, t: ops.linear_act(t["x"], t["w"], t.get("b"), act),
                     lambda t: O.linear_act_core(d(t["x"]), d(t["w"]), d(t.get("b")), act), rel(2e-5))
    return make


for N, K, act, bias in ((132, 64, "relu", True), (4, 16, "none", False), (260, 256, "gelu", True), (128, 48, "gelu", True)):
    for sym in ROWS:
        case(f"linear_act-N{N}-K{K}-rows_{sym}", "soc_linear_act_f32", _lin_act(sym, N, K, act, bias))


def _lin_act_multi(sym):
    def make(ops):
        M = rows_of(sym, 128)
        g = gen("lactm", M)
        inp = dict(x=rn(g, M, 256), pos=rn(g, M, 256), w0=rn(g, 256, 256, scale=1 / 16), b0=rn(g, 256), w1=rn(g, 132, 256, scale=1 / 16))
        return Built(inp, lambda ops, t: tuple(ops.linear_act_multi(t["x"], [(t["w0"], t["b0"]), (t["w1"], None)], t["pos"])),
                     lambda t: (O.linear_core(d(t["x"]), d(t["w0"]), d(t["b0"]), d(t["pos"])),
                                O.linear_core(d(t["x"]), d(t["w1"]), None, d(t["pos"]))), rel(3e-5))
    return make


for sym in ROWS:
    case(f"linear_act_multi-rows_{sym}", "soc_linear_act_multi_f32", _lin_act_multi(sym))


# ------------------------------------------------------------------------------------------------- K13 / K20 / K23 / K24 linear layers
def _lin_inputs(g, M, K, N, ln, res, bias, add=False, mul=False):
    inp = dict(x=rn(g, M, K, scale=1.5, shift=0.2), w=rn(g, N, K, scale=K ** -0.5))
    if bias:
        inp["b"] = rn(g, N)
    if ln:
        inp["gam"], inp["bet"] = torch.rand(K, generator=g) + 0.5, rn(g, K, scale=0.1)
    if res:
        inp["r"] = rn(g, M, N)
    if add:
        inp["a"] = rn(g, M, K, scale=0.5)
    if mul:
        inp["m"] = rn(g, M, N)
    return inp


def _lin_ref(act):
    def ref(t):
        x = d(t["x"]) + (d(t["a"]) if "a" in t else 0.0)
        K = x.shape[-1]
        h = F.layer_norm(x, (K,), d(t["gam"]), d(t["bet"]), 1e-5) if "gam" in t else x
        y = act_of(F.linear(h, d(t["w"]), d(t.get("b"))), act)
        if "m" in t:
            y = y * d(t["m"])
        return y + d(t["r"]) if "r" in t else y
    return ref


def _ln_of(t):
    return (t["gam"], t["bet"], 1e-5) if "gam" in t else None


def _ws(sym, K, N, ln, res, act, bias, mode):
    def make(ops):
        M = rows_of(sym, 32 if K <= 96 else 16)            # 16-row MFMA tiles, two per step at K <= 96 (csrc/ws_linear_split.hip RT)
        inp = _lin_inputs(gen("ws", M, K, N), M, K, N, ln, res, bias)

        def call(ops, t):
            with ops.use_matmul_mode(mode):
                return ops.ws_linear(t["x"], t["w"], t.get("b"), _ln_of(t), t.get("r"), act)
        return Built(inp, call, _lin_ref(act), rel(2e-5))
    return make


for K, N, ln, res, act, bias, mode in ((96, 288, True, False, "none", True, "split"), (128, 384, True, True, "relu", False, "split"),
                                       (256, 16, True, False, "none", True, "split"), (512, 128, False, False, "gelu", True, "split"),
                                       (384, 48, False, True, "none", True, "split"), (192, 576, True, False, "none", True, "split"),
                                       (96, 96, False, True, "none", True, "f32"), (256, 48, True, True, "gelu", True, "f32")):
    for sym in ROWS:
        case(f"ws_linear-{mode}-K{K}-N{N}-rows_{sym}", "soc_ws_linear_f32", _ws(sym, K, N, ln, res, act, bias, mode))


def _split(sym, tile, K, N, ln, res, act, bias, add, mul):
    def make(ops):
        cfg = ops.split_tile_for(128, N, K) if tile is None else tile
        M = rows_of(sym, ops.SPLIT_TILES[cfg][0])
        inp = _lin_inputs(gen("k20", M, K, N), M, K, N, ln, res, bias, add, mul)
        return Built(inp, lambda ops, t: ops.linear_split(t["x"], t["w"], t.get("b"), _ln_of(t), t.get("r"), act, t.get("a"),
                                                          t.get("m"), tile=tile), _lin_ref(act), rel(2e-5))
    return make


for K, N, ln, res, act, bias, add, mul in ((96, 288, True, False, "none", True, False, False),      # 3 K-steps, LayerNorm folded in
                                           (48, 96, False, True, "none", True, False, False),      # K = 48: a K tail inside a K-step
                                           (128, 40, False, False, "none", False, False, False),   # N % 16 != 0, narrower than any tile
                                           (1024, 132, True, True, "relu", False, False, False),   # LayerNorm at its widest, N % 16 == 4
                                           (256, 260, False, False, "gelu", True, True, True)):    # x + add in front, mul behind
    for tile in (None, 0, 1, 2, 3, 4):
        for sym in ROWS:
            case(f"linear_split-tile{tile}-K{K}-N{N}-rows_{sym}", "soc_linear_split_f32", _split(sym, tile, K, N, ln, res, act, bias, add, mul),
                 also=("soc_linear_split_pack_f32",) + (("soc_row_stats_f32",) if ln else ()))


def _split_two(sym):
    def make(ops):
        M = rows_of(sym, 128)
        inp = _lin_inputs(gen("k20two", M), M, 256, 388, False, False, True, add=True)
        return Built(inp, lambda ops, t: ops.linear_split(t["x"], t["w"], t["b"], add=t["a"], split_at=256),
                     lambda t: tuple(_lin_ref("none")(t).split([256, 132], -1)), rel(2e-5))
    return make


for sym in ROWS:
    case(f"linear_split-two_outputs-rows_{sym}", "soc_linear_split_f32", _split_two(sym), also=("soc_linear_split_pack_f32",))


def _row_stats(M, K):
    def make(ops):
        inp = dict(x=rn(gen("stats", M, K), M, K, scale=3.0, shift=5.0))

        def ref(t):
            x = d(t["x"])
            return torch.stack([x.mean(-1), 1.0 / torch.sqrt(x.var(-1, unbiased=False) + 1e-5)], -1)

        def compare(i, got, want):
            assert float((got[:, 0].double() - want[:, 0]).abs().max()) < 2e-6 * 5
            assert float((got[:, 1].double() / want[:, 1] - 1).abs().max()) < 5e-6
        return Built(inp, lambda ops, t: ops.row_stats(t["x"], 1e-5), ref, compare=compare)
    return make


for M, K in ((1, 96), (3, 1024), (77, 192), (65, 4), (513, 384)):
    case(f"row_stats-M{M}-K{K}", "soc_row_stats_f32", _row_stats(M, K))


def rows_per_group(M0, nrg):
    """Rows one workgroup row of a plan takes: 16-row tiles dealt over nrg workgroup rows."""
    return 16 * -(-(-(-M0 // 16)) // max(nrg, 1))


def _xs(sym, N, K, act, ln, res):
    def make(ops):
        nrg, _, _ = ops.xs_linear_plan(4096, N, K)
        M = rows_of(sym, rows_per_group(4096, nrg))
        inp = _lin_inputs(gen("xs", M, N, K), M, K, N, ln, res, True)
        inp["x"] = inp["x"] * 0.8
        assert ops.xs_linear_supported(torch.empty(1, K, device="cuda"), torch.empty(N, K, device="cuda"))
        return Built(inp, lambda ops, t: ops.xs_linear(t["x"], t["w"], t["b"], _ln_of(t), t.get("r"), act), _lin_ref(act),
                     scale_of(1e-5))
    return make


for N, K, act, ln, res in ((96, 1024, "relu", False, True), (64, 192, "relu", False, True), (576, 256, "none", True, False),
                           (1152, 384, "gelu", True, True), (512, 512, "none", False, True), (384, 768, "none", False, False)):
    for sym in ROWS:
        case(f"xs_linear-N{N}-K{K}-rows_{sym}", "soc_xs_linear_f32", _xs(sym, N, K, act, ln, res), also=("soc_xs_linear_pack_f32",))


def _mlp_inputs(g, M, Cw, Fh, ln, post):
    inp = dict(x=rn(g, M, Cw, scale=1.2), w1=rn(g, Fh, Cw, scale=Cw ** -0.5), b1=rn(g, Fh, scale=0.1),
               w2=rn(g, Cw, Fh, scale=Fh ** -0.5), b2=rn(g, Cw, scale=0.1))
    if ln:
        inp["gam"], inp["bet"] = torch.rand(Cw, generator=g) + 0.5, rn(g, Cw, scale=0.1)
    if post:
        inp["gam2"], inp["bet2"] = torch.rand(Cw, generator=g) + 0.5, rn(g, Cw, scale=0.1)
    return inp


def _mlp_ref(act, res, form):
    def ref(t):
        x = d(t["x"])
        Cw = x.shape[-1]
        n1 = F.layer_norm(x, (Cw,), d(t["gam"]), d(t["bet"]), 1e-5) if "gam" in t else x
        h = F.linear(n1, d(t["w1"]), d(t["b1"]))
        y = F.linear(h.relu() if act == "relu" else F.gelu(h), d(t["w2"]), d(t["b2"]))
        if res:
            y = y + (n1 if form == "residual_ln" else x)
        if "gam2" not in t:
            return y
        h2 = F.layer_norm(y, (Cw,), d(t["gam2"]), d(t["bet2"]), 1e-5)
        return (y, h2) if form == "sum" else h2
    return ref


def _mlp(M_or_sym, Cw, Fh, act, ln, res, form="plain", cut=None):
    """form: plain | post (LayerNorm behind) | sum (post + the sum in front of it) | residual_ln (the shortcut is LN(x))."""
    def make(ops):
        if isinstance(M_or_sym, str):
            nrg, _ = ops.mlp_split_plan(4096, Cw, Fh)
            M = rows_of(M_or_sym, rows_per_group(4096, nrg))
        else:
            M = M_or_sym
        post = form != "plain"
        inp = _mlp_inputs(gen("mlp", M, Cw, Fh), M, Cw, Fh, ln, post)

        def call(ops, t):
            return ops.mlp_split(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], act, _ln_of(t), residual=t["x"] if res else None, cut=cut,
                                 post_ln=(t["gam2"], t["bet2"], 1e-5) if post else None, return_sum=form == "sum",
                                 residual_ln=form == "residual_ln")
        # tests/test_gpu_kernels.py: 1e-5 |want|max for the sum, 2e-5 behind the closing LayerNorm
        tol = scale_of(1e-5) if not post else (lambda i, w: 1e-5 * absmax(w) if (form == "sum" and i == 0) else 2e-5)
        return Built(inp, call, _mlp_ref(act, res, form), tol)
    return make


_MLP_ALSO = ("soc_mlp_split_pack_f32",)
for Cw, Fh, act, ln, res, form in ((96, 384, "gelu", True, True, "plain"), (256, 2048, "relu", False, False, "plain"),
                                   (384, 1536, "gelu", True, True, "sum"), (128, 64, "gelu", False, False, "plain"),
                                   (256, 2048, "relu", True, True, "residual_ln"), (256, 1024, "relu", False, True, "post"),
                                   (512, 2048, "relu", False, False, "plain")):
    for sym in ROWS:
        case(f"mlp_split-{form}-C{Cw}-F{Fh}-rows_{sym}", "soc_mlp_split_f32", _mlp(sym, Cw, Fh, act, ln, res, form), also=_MLP_ALSO)
# whole rounds of the chip plus a split tail (the partial sums go through the workspace of soc_mlp_split_workspace_bytes)
case("mlp_split-rounds_plus_tail-M5792-C256-F2048", "soc_mlp_split_f32", _mlp(5792, 256, 2048, "relu", False, True), also=_MLP_ALSO)
case("mlp_split-rounds_plus_tail-post-M5792", "soc_mlp_split_f32", _mlp(5792, 256, 2048, "relu", False, True, "post"), also=_MLP_ALSO)
# explicit cuts: nfs > 1 sizes the workspace as nfs * M * C floats in hot_ops
for M, Cw, Fh, cut, form in ((777, 96, 384, (3, 4), "plain"), (777, 192, 768, (49, 3), "plain"), (1000, 384, 1536, (16, 3), "sum"),
                             (4099, 128, 512, (7, 2), "plain"), (1041, 256, 2048, (32, 8), "residual_ln"), (33, 256, 2048, (3, 1), "post")):
    case(f"mlp_split_variant-{form}-M{M}-C{Cw}-F{Fh}-cut{cut[0]}x{cut[1]}", "soc_mlp_split_variant_f32",
         _mlp(M, Cw, Fh, "gelu" if Cw != 256 else "relu", Cw != 256 or form == "residual_ln", True, form, cut), also=_MLP_ALSO)


# ------------------------------------------------------------------------------------------------- K15 / K16 query-side blocks
def _dec_xattn(N, Lq, rd, padding, shared_pos):
    def make(ops):
        g = gen("k15", N, Lq, rd)
        S, M, Cc = int(_LEVELS.prod(1).sum()), 8, 256
        ref = torch.rand(N, Lq, 4, rd, generator=g)
        if rd == 4:
            ref[..., 2:] *= 0.5
        inp = dict(tgt=rn(g, N, Lq, Cc), memory=rn(g, N, S, Cc), qpos=rn(g, Lq, Cc) if shared_pos else rn(g, N, Lq, Cc), ref=ref,
                   shapes=_LEVELS.clone(), lsi=_lsi(_LEVELS), w_off=rn(g, 256, Cc, scale=0.05), b_off=rn(g, 256, scale=2.0),
                   w_att=rn(g, 128, Cc, scale=0.06), b_att=rn(g, 128), w_val=rn(g, Cc, Cc, scale=0.06), b_val=rn(g, Cc, scale=0.5),
                   w_out=rn(g, Cc, Cc, scale=0.06), b_out=rn(g, Cc, scale=0.5), gamma=1 + rn(g, Cc, scale=0.1), beta=rn(g, Cc, scale=0.1))
        if padding:
            inp["pad"] = torch.rand(N, S, generator=g) < 0.3
            inp["flag"] = inp["pad"].any().to(torch.int32).reshape(1)

        def call(ops, t):
            class Lin:
                def __init__(self, w, b):
                    self.weight, self.bias = w, b

            class CA:
                d_model, n_heads, n_levels, n_points = 256, 8, 4, 4
                sampling_offsets, attention_weights = Lin(t["w_off"], t["b_off"]), Lin(t["w_att"], t["b_att"])
                value_proj, output_proj = Lin(t["w_val"], t["b_val"]), Lin(t["w_out"], t["b_out"])

            class Norm:
                weight, bias, eps = t["gamma"], t["beta"], 1e-5
            assert ops.decoder_cross_attn_supported(t["tgt"], CA, t["memory"], t["ref"])
            return ops.decoder_cross_attn(t["tgt"], t["qpos"], t["ref"], t["memory"], t["shapes"], t["lsi"], CA, Norm, t.get("pad"),
                                          t.get("flag"))

        def want(t):
            qv = d(t["tgt"]) + d(t["qpos"])
            off = F.linear(qv, d(t["w_off"]), d(t["b_off"])).view(N, Lq, M, 4, 4, 2)
            logits = F.linear(qv, d(t["w_att"]), d(t["b_att"])).view(N, Lq, M, 16)
            value = F.linear(d(t["memory"]), d(t["w_val"]), d(t["b_val"])).view(N, S, M, 32)
            sampled = O.msda_fused_core(value, t["shapes"], t["lsi"], d(t["ref"]), off, logits, t.get("pad"))
            return F.layer_norm(d(t["tgt"]) + F.linear(sampled, d(t["w_out"]), d(t["b_out"])), (Cc,), d(t["gamma"]), d(t["beta"]), 1e-5)
        return Built(inp, call, want, fixed(5e-5))
    return make


for N, Lq, rd, pad, shared in ((1, 1, 4, False, True), (3, 7, 4, True, False), (2, 33, 2, True, True), (8, 20, 2, False, True)):
    case(f"decoder_cross_attn-N{N}-Lq{Lq}-rd{rd}-pad{int(pad)}", "soc_decoder_cross_attn_f32", _dec_xattn(N, Lq, rd, pad, shared))


def _row_mlp(M, n_layers, n_out, ln, add, res):
    def make(ops):
        g = gen("rowmlp", M, n_layers, n_out)
        dims = [256] * n_layers + [n_out]
        inp = dict(x=rn(g, M, 256))
        for i in range(n_layers):
            inp[f"w{i}"], inp[f"b{i}"] = rn(g, dims[i + 1], 256, scale=0.08), rn(g, dims[i + 1], scale=0.3)
        if add:
            inp["a"] = rn(g, M, 256)
        if res:
            inp["r"] = rn(g, M, n_out)
        if ln:
            inp["gam"], inp["bet"] = 1 + rn(g, 256, scale=0.1), rn(g, 256, scale=0.1)

        def ref(t):
            h = d(t["x"]) + (d(t["a"]) if add else 0.0)
            for i in range(n_layers):
                h = F.linear(h, d(t[f"w{i}"]), d(t[f"b{i}"]))
                if i + 1 < n_layers:
                    h = h.relu()
            if res:
                h = h + d(t["r"])
            return F.layer_norm(h, (256,), d(t["gam"]), d(t["bet"]), 1e-5) if ln else h
        return Built(inp, lambda ops, t: ops.row_mlp(t["x"], [(t[f"w{i}"], t[f"b{i}"]) for i in range(n_layers)], add=t.get("a"),
                                                     residual=t.get("r"), ln=_ln_of(t)), ref, fixed(3e-5))
    return make


# one workgroup per row: the tile is one row
for n_layers, n_out, ln, add, res in ((3, 4, False, False, False), (3, 169, False, False, False), (1, 256, True, True, True),
                                      (2, 33, False, True, True)):
    for M in (1, 2, 3, 7):
        case(f"row_mlp-L{n_layers}-N{n_out}-ln{int(ln)}-M{M}", "soc_row_mlp_f32", _row_mlp(M, n_layers, n_out, ln, add, res))


# ------------------------------------------------------------------------------------------------- K17 / K18 / K19 FPN
def _gn_nchw(N, Cc, H, W, Gr, relu, with_bias):
    def make(ops):
        g = gen("gnnchw", N, Cc, H, W)
        inp = dict(x=rn(g, N, Cc, H, W, scale=2.0, shift=0.5), gam=1 + rn(g, Cc, scale=0.2), bet=rn(g, Cc, scale=0.2))
        if with_bias:
            inp["cb"] = rn(g, Cc)

        def ref(t):
            x = d(t["x"]) + (d(t["cb"]).view(1, -1, 1, 1) if with_bias else 0.0)
            y = F.group_norm(x, Gr, d(t["gam"]), d(t["bet"]), 1e-5)
            return y.relu() if relu else y

        def call(ops, t):
            assert ops.groupnorm_nchw_supported(t["x"], Gr)
            return ops.groupnorm_nchw(t["x"], t.get("cb"), t["gam"], t["bet"], Gr, 1e-5, relu=relu)
        return Built(inp, call, ref, fixed(2e-5), inplace=("x",))
    return make


# HW % 4 == 0 is required, so only one of H, W can be prime
for N, Cc, H, W, Gr, relu, wb in ((1, 8, 2, 2, 8, True, True), (1, 16, 13, 4, 8, True, True), (3, 32, 7, 12, 8, False, False),
                                  (2, 256, 4, 5, 8, True, True), (1, 8, 64, 64, 1, True, True)):
    case(f"groupnorm_nchw-N{N}-C{Cc}-{H}x{W}-G{Gr}", "soc_groupnorm_nchw_f32", _gn_nchw(N, Cc, H, W, Gr, relu, wb))


def _up_add(N, Cc, H, W, Hp, Wp, tokens, with_bias):
    def make(ops):
        g = gen("upadd", N, Cc, H, W, tokens)
        # |values| stay below 4: two f32 roundings of the add chain then stay inside the 1e-6 of the existing test
        lat, prev, b = rn(g, N, Cc, H, W, scale=0.5), rn(g, N, Cc, Hp, Wp, scale=0.5), rn(g, Cc, scale=0.5)

        def tok(x):
            return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]).contiguous()
        inp = dict(lateral=tok(lat) if tokens else lat, prev=tok(prev) if tokens else prev)
        if with_bias:
            inp["b"] = b

        def ref(t):
            want = d(lat) + F.interpolate(d(prev), size=(H, W), mode="nearest") + (d(b).view(1, -1, 1, 1) if with_bias else 0.0)
            return tok(want) if tokens else want

        def call(ops, t):
            if tokens:
                return ops.upsample_add_tokens(t["lateral"], t.get("b"), t["prev"], (H, W), (Hp, Wp))
            return ops.upsample_add_nchw(t["lateral"], t.get("b"), t["prev"])
        return Built(inp, call, ref, fixed(1e-6), inplace=("lateral",))
    return make


for N, Cc, H, W, Hp, Wp, wb in ((1, 4, 7, 5, 3, 4, True), (2, 8, 11, 13, 5, 7, True), (1, 4, 1, 1, 1, 1, False), (3, 12, 23, 37, 12, 19, True),
                                (2, 4, 9, 9, 9, 9, True)):
    case(f"upsample_add_nchw-N{N}-C{Cc}-{H}x{W}", "soc_upsample_add_nchw_f32", _up_add(N, Cc, H, W, Hp, Wp, False, wb))
    case(f"upsample_add_tokens-N{N}-C{Cc}-{H}x{W}", "soc_upsample_add_tokens_f32", _up_add(N, Cc, H, W, Hp, Wp, True, wb))
case("upsample_add_nchw-C3", "soc_upsample_add_nchw_f32", _up_add(1, 3, 7, 5, 3, 4, False, True))


def _conv(N, H, W, Cin, Cout, nchw, relu):
    def make(ops):
        g = gen("conv", N, H, W, Cin, Cout)
        inp = dict(tok=rn(g, N, H * W, Cin), taps=rn(g, Cout, 9 * Cin, scale=(2.0 / (9 * Cin)) ** 0.5), b=rn(g, Cout))

        def ref(t):
            x = d(t["tok"]).view(N, H, W, Cin).permute(0, 3, 1, 2)
            w = d(t["taps"]).view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
            y = F.conv2d(x, w, d(t["b"]), padding=1)
            y = y.relu() if relu else y
            return y if nchw else y.permute(0, 2, 3, 1).reshape(N, H * W, Cout)
        return Built(inp, lambda ops, t: ops.conv3x3_tokens(t["tok"], (H, W), t["taps"], t["b"], out_nchw=nchw, relu=relu), ref,
                     fixed(3e-5))
    return make


for N, H, W, Cin, Cout, nchw, relu in ((1, 1, 1, 32, 40, False, False), (1, 5, 7, 16, 3, True, True), (2, 11, 13, 32, 40, False, False),
                                       (1, 17, 19, 64, 32, False, True), (3, 7, 23, 16, 8, True, False), (1, 13, 5, 256, 128, False, False)):
    case(f"conv3x3-N{N}-{H}x{W}-{Cin}to{Cout}-nchw{int(nchw)}", "soc_conv3x3_tokens_f32", _conv(N, H, W, Cin, Cout, nchw, relu))


# ------------------------------------------------------------------------------------------------- K25 / K26 / K27
def _small_attn(B, L, H, Dh, mask_kind):
    def make(ops):
        g = gen("sattn", B, L, H, Dh, mask_kind)
        E = H * Dh
        inp = dict(q=rn(g, B, L, E), k=rn(g, B, L, E), v=rn(g, B, L, E))
        if mask_kind in ("keypad", "allmasked"):
            pad = torch.zeros(B, L, dtype=torch.bool)
            pad[:, L - max(1, L // 4):] = True
            if mask_kind == "allmasked":
                pad[-1, :] = True
            inp["mask"] = torch.zeros(B, 1, 1, L).masked_fill_(pad[:, None, None, :], float("-inf"))
        elif mask_kind == "full":
            inp["mask"] = rn(g, B, 1, L, L, scale=2.0)

        def ref(t):
            qd, kd, vd = (d(t[n]).view(B, L, H, Dh).transpose(1, 2) for n in "qkv")
            s = qd @ kd.transpose(-1, -2) * Dh ** -0.5
            if "mask" in t:
                s = s + d(t["mask"])
            p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)         # fully masked rows: zeros
            return (p @ vd).transpose(1, 2).reshape(B, L, E)

        def call(ops, t):
            assert ops.small_attention_supported(t["q"], H, t.get("mask"))
            return ops.small_attention(t["q"], t["k"], t["v"], H, t.get("mask"))
        return Built(inp, call, ref, rel(2e-6))
    return make


for B, L, H, Dh, kind in ((1, 1, 12, 64, "none"), (2, 7, 12, 64, "keypad"), (3, 17, 8, 32, "full"), (1, 63, 12, 64, "none"),
                          (1, 64, 12, 64, "keypad"), (2, 33, 8, 32, "allmasked")):
    case(f"small_attn-B{B}-L{L}-H{H}-D{Dh}-{kind}", "soc_small_attn_f32", _small_attn(B, L, H, Dh, kind))


def _select_pack(T, B, Q, K, h, w):
    def make(ops):
        g = gen("k26", T, B, Q, K)
        inp = dict(cls=rn(g, B, T, Q, K), masks=rn(g, T, B, Q, h, w))
        R = 1 + T * Q + T * h * w

        def call(ops, t):
            records = torch.empty(B, R, dtype=torch.float32, device=t["cls"].device)     # guarded: an unwritten field shows up
            ops.select_pack(t["cls"].transpose(0, 1), t["masks"], records)               # [T,B,Q,K], the model's transposed view
            return records

        def ref(t):
            cls = d(t["cls"]).transpose(0, 1)
            idx = cls.sigmoid().mean(0).max(-1)[0].argmax(-1)                             # [B]
            return torch.stack([torch.cat([idx[b:b + 1].double(), cls[:, b, :, 0].reshape(-1),
                                           d(t["masks"])[:, b, idx[b]].reshape(-1)]) for b in range(B)])
        return Built(inp, call, ref, fixed(0.0))
    return make


for T, B, Q, K, h, w in ((1, 1, 1, 1, 1, 1), (3, 2, 7, 3, 5, 9), (8, 4, 20, 1, 13, 17), (36, 1, 20, 1, 3, 7)):
    case(f"select_pack-T{T}-B{B}-Q{Q}-K{K}-{h}x{w}", "soc_select_pack_f32", _select_pack(T, B, Q, K, h, w))


def _davis(Gn, P, T, H, W, r, use_void, pairs):
    def make(ops):
        from tests.test_gpu_davis_eval import oracle_counts
        rng = np.random.default_rng(Gn * 100 + H)

        def blobs(n):
            m = rng.integers(0, n + 1, (T, -(-H // 4), -(-W // 4))).repeat(4, 1).repeat(4, 2)[:, :H, :W].astype(np.uint8)
            return m
        gt = blobs(Gn)
        gt[rng.uniform(size=gt.shape) < 0.03] = 255
        inp = dict(gt=torch.from_numpy(gt), pred=torch.from_numpy(blobs(max(P, 1))))
        return Built(inp, lambda ops, t: ops.davis_jf_counts(t["gt"], t["pred"], Gn, P, r, use_void, pairs),
                     lambda t: torch.from_numpy(oracle_counts(t["gt"].numpy(), t["pred"].numpy(), Gn, P, r, use_void, pairs)),
                     fixed(0.0))
    return make


for Gn, P, T, H, W, r, uv, pairs in ((1, 1, 1, 3, 5, 1, True, True), (2, 2, 1, 13, 17, 2, True, True), (3, 2, 2, 45, 83, 3, True, False),
                                     (2, 3, 3, 31, 67, 5, False, True), (1, 2, 1, 7, 129, 1, True, True)):
    case(f"davis_jf_counts-G{Gn}-P{P}-T{T}-{H}x{W}-r{r}-pairs{int(pairs)}", "soc_davis_jf_counts_u8", _davis(Gn, P, T, H, W, r, uv, pairs))


# ------------------------------------------------------------------------------------------------- the table, run
def _judge(b: Built):
    def compare_all(i, got, want):
        if b.compare is not None:
            return b.compare(i, got, want)
        bound = b.tol(i, want)
        assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
        if not got.numel():
            return
        if bound == 0.0:        # bit-exact against the f64 result rounded once to the output's type
            assert torch.equal(got, want.to(got.dtype)), f"not bit-exact: max |diff| {float((got.double() - want.double()).abs().max()):.3e}"
            return
        err = float((got.double() - want.double()).abs().max())
        print(f"    output {i}: max |got - f64| = {err:.3e}, bound {bound:.3e}")
        assert err < bound, f"max |got - f64| = {err:.3e} >= {bound:.3e}"
    return compare_all


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_memory_contract(ops, c):
    b = c.make(ops)
    G.check_contract(b.inputs, lambda t: b.call(ops, t), "cuda", entry=(c.entry,) + c.also, inplace=b.inplace, reference=b.ref,
                     compare=_judge(b))


# ------------------------------------------------------------------------------------------------- hostile neighbours
def test_mlp_split_writes_only_its_slice_of_a_poisoned_buffer(ops):
    """mlp_split(out=buf[:M]) inside a NaN-filled buffer: the rows behind M stay NaN bit for bit, for the planned launch
    (whole rounds + split tail) and for explicit cuts with and without split hidden ranges."""
    for M, Cw, Fh, cut in ((5792, 256, 2048, None), (5792, 256, 2048, (46, 4)), (777, 96, 384, (3, 4)), (1000, 384, 1536, (16, 1))):
        b = _mlp(M, Cw, Fh, "gelu", True, True, cut=cut)(ops)
        t = {k: v.cuda() for k, v in b.inputs.items()}
        buf = torch.full((M + 300, Cw), float("nan"), device="cuda")
        poison = buf.view(torch.int32).clone()
        got = ops.mlp_split(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], "gelu", _ln_of(t), residual=t["x"], out=buf[:M], cut=cut)
        want = b.ref(b.inputs)
        assert float((got.double().cpu() - want).abs().max()) < 1e-5 * absmax(want), (M, Cw, Fh, cut)
        assert torch.equal(buf.view(torch.int32)[M:], poison[M:]), (M, Cw, Fh, cut)
        assert bool(torch.isfinite(buf[:M]).all())


# ------------------------------------------------------------------------------------------------- aliasing clauses of the header
def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("alias", ["x", "y"])
@pytest.mark.parametrize("rows,Cc", [(37, 96), (17, 256), (9, 768), (5, 2048)])
def test_alias_add_layernorm_out_sum(ops, alias, rows, Cc):
    """soc_add_layernorm_f32: out_sum may alias x or y."""
    from neurips2023_soc_amd import _lib
    g = gen("alias_aln", rows, Cc)
    x, y, w, b = (v.cuda() for v in (rn(g, rows, Cc, scale=3.0), rn(g, rows, Cc), rn(g, Cc), rn(g, Cc)))
    s0, n0 = ops.add_layernorm(x, y, w, b, 1e-5)
    xa, ya = x.clone(), y.clone()
    n1 = torch.full_like(x, float("nan"))
    tgt = xa if alias == "x" else ya
    _lib.check(_lib.load().soc_add_layernorm_f32(_ptr(xa), _ptr(ya), _ptr(w), _ptr(b), _ptr(tgt), _ptr(n1), rows, Cc, 1e-5, ops._stream()),
               "soc_add_layernorm_f32")
    assert _bits_equal(tgt, s0) and _bits_equal(n1, n0)
    assert _bits_equal(ya if alias == "x" else xa, y if alias == "x" else x)         # the other operand is untouched


@pytest.mark.parametrize("mode", ["split", "f32"])
@pytest.mark.parametrize("M,K,N,ln,act", [(3001, 128, 384, True, "relu"), (37, 96, 96, False, "none"), (1025, 384, 48, False, "gelu"),
                                          (4099, 256, 256, True, "none")])
def test_alias_ws_linear_out_residual(ops, mode, M, K, N, ln, act):
    """soc_ws_linear_f32: out may alias residual (ragged M: the clamped tail lanes read the aliased buffer)."""
    from neurips2023_soc_amd import _lib
    t = {k: v.cuda() for k, v in _lin_inputs(gen("alias_ws", M, K, N), M, K, N, ln, True, True).items()}
    with ops.use_matmul_mode(mode):
        want = ops.ws_linear(t["x"], t["w"], t["b"], _ln_of(t), t["r"], act)
        buf = t["r"].clone()
        _lib.check(_lib.load().soc_ws_linear_f32(_ptr(t["x"]), _ptr(t.get("gam")), _ptr(t.get("bet")), 1e-5, _ptr(t["w"]), _ptr(t["b"]),
                                                 _ptr(buf), _ptr(buf), M, N, K, {"none": 0, "relu": 1, "gelu": 2}[act],
                                                 int(ops.k13_split_enabled()), ops._stream()), "soc_ws_linear_f32")
    assert _bits_equal(buf, want)


@pytest.mark.parametrize("alias", ["residual", "mul"])
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("M,K,N", [(777, 256, 260), (129, 96, 288), (257, 48, 40)])
def test_alias_linear_split_out_residual_or_mul(ops, alias, tile, M, K, N):
    """soc_linear_split_f32: out may alias residual or mul."""
    from neurips2023_soc_amd import _lib
    t = {k: v.cuda() for k, v in _lin_inputs(gen("alias_k20", M, K, N), M, K, N, False, True, True, mul=True).items()}
    want = ops.linear_split(t["x"], t["w"], t["b"], None, t["r"], "gelu", None, t["m"], tile=tile)
    packed, bias, _ = ops.split_pack(t["w"], t["b"])
    r, m = t["r"].clone(), t["m"].clone()
    out = r if alias == "residual" else m
    _lib.check(_lib.load().soc_linear_split_f32(_ptr(t["x"]), None, None, None, _ptr(packed), _ptr(bias), _ptr(r), _ptr(m), _ptr(out), None, 0,
                                                M, N, K, 2, tile, ops._stream()), "soc_linear_split_f32")
    assert _bits_equal(out, want)
    assert _bits_equal(m if alias == "residual" else r, t["m"] if alias == "residual" else t["r"])


@pytest.mark.parametrize("N,Cc,H,W,Gr", [(3, 32, 7, 12, 8), (1, 16, 13, 4, 8), (2, 256, 4, 5, 8), (1, 8, 64, 64, 1)])
def test_alias_groupnorm_nchw_y_x(ops, N, Cc, H, W, Gr):
    """soc_groupnorm_nchw_f32: y may alias x (what hot_ops.groupnorm_nchw always does) -- against the two-buffer call."""
    from neurips2023_soc_amd import _lib
    g = gen("alias_gn", N, Cc, H, W)
    x, cb, gam, bet = (v.cuda() for v in (rn(g, N, Cc, H, W, scale=2.0, shift=0.5), rn(g, Cc), 1 + rn(g, Cc, scale=0.2), rn(g, Cc, scale=0.2)))
    y = torch.full_like(x, float("nan"))
    keep = x.clone()
    _lib.check(_lib.load().soc_groupnorm_nchw_f32(_ptr(x), _ptr(cb), _ptr(gam), _ptr(bet), _ptr(y), N, Cc, H * W, Gr, 1e-5, 1, ops._stream()),
               "soc_groupnorm_nchw_f32")
    assert _bits_equal(x, keep)
    assert _bits_equal(ops.groupnorm_nchw(x, cb, gam, bet, Gr, 1e-5, relu=True), y)


@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("N,Cc,H,W,Hp,Wp", [(1, 4, 7, 5, 3, 4), (3, 12, 23, 37, 12, 19), (2, 8, 11, 13, 5, 7), (2, 4, 9, 9, 9, 9)])
def test_alias_upsample_add_y_lateral(ops, tokens, N, Cc, H, W, Hp, Wp):
    """soc_upsample_add_tokens_f32 and soc_upsample_add_nchw_f32: y may alias lateral (what hot_ops always does) -- against the
    two-buffer call."""
    from neurips2023_soc_amd import _lib
    b = _up_add(N, Cc, H, W, Hp, Wp, tokens, True)(ops)
    t = {k: v.cuda() for k, v in b.inputs.items()}
    y = torch.full_like(t["lateral"], float("nan"))
    keep = t["lateral"].clone()
    fn = _lib.load().soc_upsample_add_tokens_f32 if tokens else _lib.load().soc_upsample_add_nchw_f32
    _lib.check(fn(_ptr(t["lateral"]), _ptr(t["b"]), _ptr(t["prev"]), _ptr(y), N, Cc, H, W, Hp, Wp, ops._stream()), "soc_upsample_add")
    assert _bits_equal(t["lateral"], keep)
    assert _bits_equal(b.call(ops, t), y)


# ------------------------------------------------------------------------------------------------- row isolation
# One input row NaN, then +Inf: every other output row keeps its bits, the poisoned row is non-finite.  Rows poisoned in
# turn: the first, the last, the last row of a full tile, the first row of the ragged tail.  The cases end in no activation
# or GELU: the kernels' ReLU is fmaxf(v, 0), which maps NaN to 0, so "the poisoned row is non-finite" is not defined behind it.
def _isolation(ops, name):
    """(CPU inputs, call(ops, t), rows M, tile t) of the kernel's isolation case; M = 2 t + 3: two full tiles and a ragged tail."""
    if name == "ws_linear":
        t_ = 32
        M = 2 * t_ + 3
        return _lin_inputs(gen("iso", name), M, 96, 288, True, True, True), \
            (lambda ops, t: ops.ws_linear(t["x"], t["w"], t["b"], _ln_of(t), t["r"], "gelu")), M, t_
    if name == "ws_linear_f32":
        t_ = 16
        M = 2 * t_ + 3

        def call(ops, t):
            with ops.use_matmul_mode("f32"):
                return ops.ws_linear(t["x"], t["w"], t["b"], _ln_of(t), t["r"], "gelu")
        return _lin_inputs(gen("iso", name), M, 256, 48, True, True, True), call, M, t_
    if name == "linear_split":
        t_ = ops.SPLIT_TILES[ops.split_tile_for(128, 288, 96)][0]
        M = 2 * t_ + 3
        return _lin_inputs(gen("iso", name), M, 96, 288, True, True, True), \
            (lambda ops, t: ops.linear_split(t["x"], t["w"], t["b"], _ln_of(t), t["r"], "gelu")), M, t_
    if name == "xs_linear":
        t_ = rows_per_group(4096, ops.xs_linear_plan(4096, 576, 256)[0])
        M = 2 * t_ + 3
        return _lin_inputs(gen("iso", name), M, 256, 576, True, True, True), \
            (lambda ops, t: ops.xs_linear(t["x"], t["w"], t["b"], _ln_of(t), t["r"], "gelu")), M, t_
    if name == "mlp_split":
        t_ = rows_per_group(4096, ops.mlp_split_plan(4096, 96, 384)[0])
        M = 2 * t_ + 3
        return _mlp_inputs(gen("iso", name), M, 96, 384, True, False), \
            (lambda ops, t: ops.mlp_split(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], "gelu", _ln_of(t), residual=t["x"])), M, t_
    if name == "linear_act":
        t_ = 128
        M = 2 * t_ + 3
        return _lin_inputs(gen("iso", name), M, 64, 132, False, False, True), \
            (lambda ops, t: ops.linear_act(t["x"], t["w"], t["b"], "gelu")), M, t_
    if name == "linear_small":
        t_ = 16
        M = 2 * t_ + 3
        return _lin_inputs(gen("iso", name), M, 256, 169, False, False, True), \
            (lambda ops, t: ops.linear_small(t["x"], t["w"], t["b"], None, False)), M, t_
    if name == "row_mlp":
        b = _row_mlp(7, 1, 256, True, True, True)(ops)
        return b.inputs, b.call, 7, 3
    if name == "add_layernorm":
        t_ = aln_tile(256)
        M = 2 * t_ + 3
        g = gen("iso", name)
        return dict(x=rn(g, M, 256), y=rn(g, M, 256), w=rn(g, 256), b=rn(g, 256)), \
            (lambda ops, t: ops.add_layernorm(t["x"], t["y"], t["w"], t["b"], 1e-5)[1]), M, t_
    raise KeyError(name)


ROW_KERNELS = ("ws_linear", "ws_linear_f32", "linear_split", "xs_linear", "mlp_split", "linear_act", "linear_small", "row_mlp",
               "add_layernorm")


def _poisoned_rows(M, t_):
    return {"first": 0, "last": M - 1, "last_of_full_tile": t_ - 1, "first_of_tail": (M // t_) * t_ if M % t_ else M - t_}


def _assert_isolated(clean, got, row_mask, what):
    """row_mask [rows] bool: the rows that may change.  Every other row bit-identical, every poisoned row non-finite."""
    c2, g2 = clean.reshape(row_mask.numel(), -1), got.reshape(row_mask.numel(), -1)
    same = (c2.view(torch.int32) == g2.view(torch.int32)).all(-1)
    leaked = (~same & ~row_mask).nonzero().flatten()
    assert leaked.numel() == 0, f"{what}: {leaked.numel()} clean rows changed, first {leaked[:8].tolist()}"
    finite = torch.isfinite(g2).all(-1)
    assert not bool((finite & row_mask).any()), f"{what}: poisoned rows {(finite & row_mask).nonzero().flatten()[:8].tolist()} came out finite"


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("name", ROW_KERNELS)
def test_row_isolation(ops, name, value):
    inputs, call, M, t_ = _isolation(ops, name)
    t = {k: v.cuda() for k, v in inputs.items()}
    clean = call(ops, t).clone()
    assert bool(torch.isfinite(clean).all())
    for where, row in _poisoned_rows(M, t_).items():
        bad = dict(t)
        bad["x"] = t["x"].clone()
        bad["x"][row] = value
        got = call(ops, bad)
        mask = torch.zeros(M, dtype=torch.bool, device="cuda")
        mask[row] = True
        _assert_isolated(clean, got, mask, f"{name}, {where} row {row} of {M} (tile {t_}) = {value}")


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("H,W,Cc", [(11, 13, 96), (8, 10, 128)])
def test_row_isolation_patch_merge_layernorm(ops, value, H, W, Cc):
    """K11: an input token feeds exactly one output row (its 2 x 2 neighbourhood); four output rows per workgroup."""
    g = gen("iso_pm", H, W, Cc)
    x, w, b = (v.cuda() for v in (rn(g, 1, 2, H, W, Cc), rn(g, 4 * Cc), rn(g, 4 * Cc)))
    clean = ops.patch_merge_layernorm(x, w, b, 1e-5).clone()
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    rows = 2 * H2 * W2
    for where, orow in _poisoned_rows(rows, 4).items():
        f, rem = divmod(orow, H2 * W2)
        oy, ox = divmod(rem, W2)
        bad = x.clone()
        bad[0, f, 2 * oy, 2 * ox] = value
        got = ops.patch_merge_layernorm(bad, w, b, 1e-5)
        mask = torch.zeros(rows, dtype=torch.bool, device="cuda")
        mask[orow] = True
        _assert_isolated(clean, got, mask, f"patch_merge {H}x{W}, {where} output row {orow} = {value}")


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("N,Cc,Gr", [(3, 256, 32), (2, 64, 8)])
def test_row_isolation_groupnorm_tokens(ops, value, N, Cc, Gr):
    """K10: the unit is (frame, group): poisoning one row's channels of one group spoils that (n, group) and nothing else."""
    t_ = gn_tile(Cc)
    S = 2 * t_ + 3
    g = gen("iso_gn", N, Cc)
    x, w, b = (v.cuda() for v in (rn(g, N, S, Cc), rn(g, Cc), rn(g, Cc)))
    clean = ops.groupnorm_tokens(x, w, b, Gr, 1e-5).clone()
    cpg = Cc // Gr
    for where, row in _poisoned_rows(S, t_).items():
        for n, grp in ((0, 0), (N - 1, Gr - 1)):
            bad = x.clone()
            bad[n, row, grp * cpg:(grp + 1) * cpg] = value
            got = ops.groupnorm_tokens(bad, w, b, Gr, 1e-5)
            # view as units: [N, S, G, cpg] -> [N, G, S * cpg]
            units = lambda v: v.view(N, S, Gr, cpg).permute(0, 2, 1, 3).reshape(N * Gr, -1)      # noqa: E731
            mask = torch.zeros(N * Gr, dtype=torch.bool, device="cuda")
            mask[n * Gr + grp] = True
            _assert_isolated(units(clean), units(got), mask, f"groupnorm_tokens, {where} row {row} of {S}, unit ({n}, {grp}) = {value}")
