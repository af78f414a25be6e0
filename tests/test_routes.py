"""The kernel every pixel-sized linear layer takes, pinned per BASELINE configuration.

CPU: `routes.table()` (stand-in tensors through the real dispatch predicates) against tests/golden/routes.json -- a threshold
change that silently sends a layer back to the library GEMM fails here and has to be acknowledged by re-generating the golden
(`python -m neurips2023_soc_amd.routes --write`).  GPU: the launches a real forward records are the ones the table names."""
import json

import pytest
import torch

from neurips2023_soc_amd import routes


def test_route_table_matches_the_golden():
    with open(routes.GOLDEN) as f:
        want = json.load(f)
    got = routes.all_tables()
    assert set(got) == set(want)
    for cfg in want:
        assert got[cfg] == want[cfg], (cfg, {k: (got[cfg].get(k), want[cfg].get(k))
                                             for k in set(got[cfg]) | set(want[cfg]) if got[cfg].get(k) != want[cfg].get(k)})


def test_route_table_needs_no_native_library(monkeypatch):
    """Routing reads shapes, dtypes and devices only: on a checkout without libsoc_hip.so (it is git-ignored) and without hipcc the
    table still comes out (mlp_split_supported used to load the library for soc_mlp_split_max_hidden)."""
    from neurips2023_soc_amd import _lib

    def no_library(*a, **k):
        raise _lib.SocHipError("libsoc_hip.so is missing (test)")
    monkeypatch.setattr(_lib, "load", no_library)
    with open(routes.GOLDEN) as f:
        want = json.load(f)
    assert routes.table("video-swin-t", 8, 360, 640) == want["video-swin-t T=8 360x640"]
    assert routes.table("video-swin-t", 8, 360, 640, 10) == want["video-swin-t T=8 360x640 x10 clips"]


def test_headline_config_keeps_its_hand_written_kernels():
    """The BASELINE headline (Swin-T, T = 8, 360 x 640): every MLP of stages 0-2 and the encoder's feed-forward block on K23,
    qkv / proj of stages 0-1 on K13b, of stages 2-3 and the encoder's value / output projections on K24; what is left to the library is the
    list below (hidden width 3072 of stage 3, the K = 1536 reduction, the coarse levels' narrow projections)."""
    t = routes.table("video-swin-t", 8, 360, 640)
    assert [t[f"swin{s}.mlp"] for s in range(3)] == ["k23"] * 3 and t["encoder.ffn"] == "k23"
    assert all(t[f"swin{s}.{n}"] == "k13b" for s in range(2) for n in ("qkv", "proj"))
    assert all(t[f"swin{s}.{n}"] == "k24" for s in (2, 3) for n in ("qkv", "proj")) and t["swin3.fc1"] == "k24"
    assert t["encoder.value_proj"] == t["encoder.output_proj"] == "k24" and t["encoder.offsets|weights"] == "k20"
    library = sorted(k for k, v in t.items() if v == "library")
    assert library == ["input_proj3", "merge2", "swin3.fc2", "vlf2.out*tgt", "vlf2.q", "vlf3.out*tgt", "vlf3.q"], library


def test_f32_mode_sends_nothing_to_the_bf16_kernels():
    from neurips2023_soc_amd import hot_ops
    with hot_ops.use_matmul_mode("f32"):
        t = routes.table("video-swin-t", 8, 360, 640)
    assert hot_ops.matmul_mode() == "split"
    assert all(v not in ("k23", "k20", "k24") for v in t.values()), t  # ("k13b" sites run the f32-MFMA form of K13 then)


def _expected_flow(mode: str, C: int, rows: int) -> str:
    """The row counts at which a stage of width C changes its flow, as read off the code before plan_stage existed."""
    if mode == "f32":
        return "ws" if C <= 256 and rows >= 16384 else "k5"
    if C in (768, 1024):
        return "k5" if rows < 1024 else "k20" if C == 1024 and rows >= 16384 else "k24"
    if rows < 4096:
        return "k5"
    if C in (384, 512) or rows < 16384:
        return "k23"
    return "k20" if C == 256 and rows * 256 >= 5_500_000 else "ws"      # K20 fills the chip from 21 485 rows of 256 columns


@pytest.mark.parametrize("mode", ["split", "f32"])
def test_plan_and_table_agree_on_both_sides_of_every_boundary(mode):
    """plan_stage (what BasicLayer.forward executes) and routes.table (what the golden pins) name the same flow for every width
    on each side of every row-count boundary, in both modes, and every route either of them names is a known label."""
    from types import SimpleNamespace as NS
    from neurips2023_soc_amd import hot_ops, linear_routes as LR
    lin = lambda n, k: NS(weight=LR.Stand(n, k), bias=LR.Stand(n))      # noqa: E731
    with hot_ops.use_matmul_mode(mode):
        for rows in (1023, 1024, 4095, 4096, 16383, 16384, 21484, 21485, 21504):
            # a clip of `rows` frames of 4 x 4 pixels: one token per frame at every stage, so each stage sees `rows` rows
            tables = {b: routes.table(b, rows, 4, 4) for b in ("video-swin-t", "video-swin-b")}
            for b, t in tables.items():
                assert all(v in (LR.FLOWS if k.endswith(".flow") else LR.LABELS) for k, v in t.items()), (b, rows, t)
                for s in range(4):
                    C = routes.SWIN_CONFIGS[b]["embed_dim"] * 2 ** s
                    blk = NS(attn=NS(qkv=lin(3 * C, C), proj=lin(C, C)), mlp=NS(fc1=lin(4 * C, C), fc2=lin(C, 4 * C)))
                    plan = LR.plan_stage(LR.Stand(1, 1, rows, 1, C), blk)
                    assert plan.flow == t[f"swin{s}.flow"] == _expected_flow(mode, C, rows), (mode, C, rows, plan)
                    assert {k: v for k, v in plan._asdict().items() if v is not None} == \
                        {k.split(".")[1]: v for k, v in t.items() if k.startswith(f"swin{s}.")}, (mode, C, rows)
                    assert (plan.mlp == "k23") == (plan.fc1 is None) == (plan.fc2 is None)
                    assert all(v in LR.LABELS for v in plan[1:] if v is not None)


def test_an_explicit_library_route_stays_on_the_library(monkeypatch):
    """A caller that holds a plan gets the kernel the plan names: with route="library" the layer is the library GEMM with a pass
    for mul and for the shortcut behind it (a "ws" stage's fc2 beyond K13: x + fc2(h)), and route_linear is not asked again --
    it could send the bare layer elsewhere (K24 for Swin-T stage 1's fc2 with SOC_SPLIT_OFF=mlp)."""
    import torch.nn.functional as F
    from neurips2023_soc_amd import fused

    def asked(*a, **k):
        raise AssertionError("route_linear asked although the caller named a route")
    monkeypatch.setattr(fused, "route_linear", asked)
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(3, 7, 32, generator=g), torch.randn(24, 32, generator=g), torch.randn(24, generator=g)
    r, m, pos = torch.randn(3, 7, 24, generator=g), torch.randn(3, 7, 24, generator=g), torch.randn(7, 32, generator=g)
    assert torch.equal(fused.linear(x, w, b, residual=r, route="library"), r + F.linear(x, w, b))
    assert torch.equal(fused.linear(x, w, b, add=pos, mul=m, residual=r, act="relu", route="library"),
                       F.relu(F.linear(x + pos, w, b)) * m + r)
    assert torch.equal(fused.linear(x, w, None, mul=m, act="gelu", route="library"), F.gelu(F.linear(x, w)) * m)
    with pytest.raises(ValueError):
        fused.linear(x, w, b, ln=(torch.ones(32), torch.zeros(32), 1e-5), route="library")
    with pytest.raises(AssertionError, match="route_linear asked"):
        fused.linear(x, w, b, residual=r)


@pytest.mark.parametrize("mode", ["split", "f32"])
def test_a_layernorm_in_front_goes_to_k20_or_nowhere(mode):
    """route_linear(ln=True), the form no stage plan covers: K20 where it can fold the LayerNorm and split_wins, else "library",
    which fused.linear refuses for a LayerNorm; never a kernel whose rule was measured on normalised inputs only."""
    from neurips2023_soc_amd import hot_ops, linear_routes as LR
    with hot_ops.use_matmul_mode(mode):
        for K in (96, 192, 256, 384, 768, 1024, 2048):
            for rows in (512, 4096, 16384, 40000, 250000):
                for N in (K, 3 * K, 256):
                    for kw in ({}, {"act": "gelu"}, {"residual": LR.Stand(rows, N)}):
                        x, w = LR.Stand(rows, K), LR.Stand(N, K)
                        got = LR.route_linear(x, w, LR.Stand(N), ln=True, **kw)
                        passes = 1 + len(kw)
                        site = "gelu" if "act" in kw else "res" if kw else "plain"
                        want = ("k20" if hot_ops.linear_split_supported(x, w, True) and LR.split_wins(rows, N, K, passes, site)
                                else "library")
                        assert got == want, (mode, rows, N, K, kw, got)
        assert LR.route_linear(LR.Stand(28800, 192), LR.Stand(576, 192), LR.Stand(576), ln=True) == \
            ("k20" if mode == "split" else "library")


def _site_shapes(backbone: str, T: int, H: int, W: int):
    """{site of routes.table: (rows, N, K) of its launch} -- for a K23 site (width, hidden) in place of (N, K), for the stacked
    offsets | weights pair the 256 + 128 rows of both layers."""
    d = routes.SWIN_CONFIGS[backbone]["embed_dim"]
    h, w = -(-H // 4), -(-W // 4)
    out, rows, enc = {}, [], 0
    for s in range(4):
        C = d * 2 ** s
        rows.append(T * h * w)
        out.update({f"swin{s}.qkv": (rows[s], 3 * C, C), f"swin{s}.proj": (rows[s], C, C), f"swin{s}.mlp": (rows[s], C, 4 * C),
                    f"swin{s}.fc1": (rows[s], 4 * C, C), f"swin{s}.fc2": (rows[s], C, 4 * C)})
        h, w = -(-h // 2), -(-w // 2)
        if s < 3:
            out[f"merge{s}"] = (T * h * w, 2 * C, 4 * C)
        if s:
            out[f"input_proj{s}"] = (rows[s], 256, C)
            out[f"vlf{s}.q"] = out[f"vlf{s}.out*tgt"] = (rows[s], 256, 256)
    enc = sum(rows[1:]) + T * h * w                     # h, w: the extra stride-64 level by now
    out.update({"encoder.value_proj": (enc, 256, 256), "encoder.output_proj": (enc, 256, 256),
                "encoder.offsets|weights": (enc, 384, 256), "encoder.ffn": (enc, 256, 2048)})
    return out, rows, enc


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["split", "f32"])
def test_recorded_launches_are_the_ones_the_table_names(mode):
    """One eager forward of the headline configuration with the call recorders on: every site of the table shows up with its
    (rows, N, K) in the recorded calls of the kernel the table names (K13b / K20 / K23 / K24) and of no other of the four."""
    import neurips2023_soc_amd as S
    from neurips2023_soc_amd import hot_ops, weights as W
    T, H, Wd, L = 8, 360, 640, 10
    dev = torch.device("cuda")
    model, _, _ = S.build_model(S.default_args("video-swin-t", text_encoder_random_init=True))
    W.load_synthetic(model, 2023)
    model = model.to(dev).eval()
    model.matmul_mode = mode
    clip = W.synthetic_clip(1, T, H, Wd).to(dev)
    ids = W.synthetic_token_ids(1, L)
    text = {"input_ids": ids.to(dev), "attention_mask": torch.ones_like(ids).to(dev)}
    pad = torch.zeros(T, 1, H, Wd, dtype=torch.bool, device=dev)
    targets = [[{"size": (H, Wd)}] for _ in range(T)]
    fresh = lambda: S.NestedTensor(clip[:, None], pad, unpadded=True)     # noqa: E731  (the forward rewrites its layout in place)
    model(fresh(), None, text, targets)                     # warm-up (weight images, caches)
    for rec in (hot_ops.record_ws_linear_calls, hot_ops.record_linear_split_calls, hot_ops.record_mlp_split_calls,
                hot_ops.record_xs_linear_calls):
        rec(True)
    model(fresh(), None, text, targets)
    k13 = {(c["x"].numel() // c["weight"].shape[1], *c["weight"].shape) for c in hot_ops.record_ws_linear_calls(False)}
    k20 = {(c["x"].numel() // c["weight"].shape[1], *c["weight"].shape) for c in hot_ops.record_linear_split_calls(False)}
    k23 = {(c["x"].numel() // c["w1"].shape[1], c["w1"].shape[1], c["w1"].shape[0]) for c in hot_ops.record_mlp_split_calls(False)}
    k24 = {(c["x"].numel() // c["weight"].shape[1], *c["weight"].shape) for c in hot_ops.record_xs_linear_calls(False)}
    with hot_ops.use_matmul_mode(mode):
        t = routes.table("video-swin-t", T, H, Wd)
    shapes, rows, enc = _site_shapes("video-swin-t", T, H, Wd)
    assert rows == [T * 90 * 160, T * 45 * 80, T * 23 * 40, T * 12 * 20] and enc == T * (45 * 80 + 23 * 40 + 12 * 20 + 6 * 10)
    # sites of one shape (a fusion block's two projections, the encoder's two) may take different kernels: a shape is found in
    # the recorders of exactly the kernels the table names for it; "library", "k7" and "k12" sites are in none of the four
    seen = {"k13b": k13, "k20": k20, "k23": k23, "k24": k24}
    for site, route in t.items():
        if site.endswith(".flow"):
            continue
        named = {t[other] for other in t if shapes.get(other) == shapes[site]} & set(seen)
        found = {kernel for kernel, calls in seen.items() if shapes[site] in calls}
        assert found == named, (site, route, shapes[site], found)
    if mode == "f32":
        assert not k20 and not k23 and not k24
        return
    for s, C in enumerate((96, 192, 384)):
        assert (rows[s], C, 4 * C) in k23, (s, sorted(k23))
    for s, C in enumerate((96, 192)):
        assert (rows[s], 3 * C, C) in k13 and (rows[s], C, C) in k13, (s, sorted(k13))
    for s, C in ((2, 384), (3, 768)):
        assert (rows[s], 3 * C, C) in k24 and (rows[s], C, C) in k24, (s, sorted(k24))
    assert (enc, 256, 2048) in k23 and (enc, 256, 256) in k24 and (enc, 384, 256) in k20      # FFN, value / output proj, offsets | weights
    assert t["encoder.value_proj"] == t["encoder.output_proj"] == "k24"
    assert (rows[1], 192, 384) in k24 and (rows[2], 384, 768) in k24      # merge0, merge1
    assert t["swin3.fc1"] == "k24" and (rows[3], 3072, 768) in k24
