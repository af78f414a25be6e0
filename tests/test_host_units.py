"""CPU unit tests of small host-side pieces: weight generator determinism, positional encodings,
config flattening, and the rule that the product package never touches the oracle."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from neurips2023_soc_amd import config, position_encoding as PE, weights as W
from neurips2023_soc_amd.nested_tensor import NestedTensor, inverse_sigmoid
from oracle import soc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weight_generator_is_pinned():
    """Integer-only generator: these digests must be identical on every platform, otherwise the
    goldens (made with the reference in the build container) and the GPU box would see different
    checkpoints."""
    z = W.unit_normal(2023, "backbone.0.body.layers.0.blocks.0.attn.qkv.weight", 1000)
    assert hashlib.sha256(z.tobytes()).hexdigest()[:16] == "1300275cd76671df"   # recorded in the build container
    assert abs(float(z.mean())) < 0.15 and 0.85 < float(z.std()) < 1.15
    # chunking must not change the stream
    big = W.unit_normal(1, "k", (1 << 18) + 17)
    assert np.array_equal(big[:100], W.unit_normal(1, "k", 100))
    ids = W.synthetic_token_ids(1, 10)
    assert ids.shape == (1, 10) and ids[0, 0] == 0 and ids[0, -1] == 2 and int(ids.min()) >= 0
    clip = W.synthetic_clip(3, 2, 8, 8)
    assert clip.shape == (2, 3, 8, 8) and clip.dtype == torch.float32


def test_weight_generator_known_values():
    # literal values recorded when the goldens were generated (seed 2023)
    z = W.unit_normal(2023, "query_embed.weight", 4)
    ref = W.unit_normal(2023, "query_embed.weight", 8)[:4]
    assert np.array_equal(z, ref)
    t = W.make_tensor(2023, "transformer.decoder.bbox_embed.0.layers.2.bias", (4,))
    u = W.make_tensor(2023, "bbox_embed.0.layers.2.bias", (4,))
    assert torch.equal(t, u)          # aliased module -> identical tensors
    assert float(u[2]) < -1.5 and float(u[3]) < -1.5   # w,h logits biased to -2


def test_position_encodings_match_oracle():
    mask = torch.zeros(2, 5, 7, dtype=torch.bool)
    mask[1, :, 5:] = True
    mask[1, 4:, :] = True
    a = PE.PositionEmbeddingSine2D(128, normalize=True)(NestedTensor(torch.zeros(2, 256, 5, 7), mask))
    assert torch.allclose(a, O.sine_pos_2d(mask), atol=1e-6)
    tm = torch.tensor([[False, False, False, True, True]])
    b = PE.PositionEmbeddingSine1D(256, normalize=True)(NestedTensor(torch.zeros(1, 256, 5), tm))
    assert torch.allclose(b, O.sine_pos_1d(tm), atol=1e-6)


def test_inverse_sigmoid_and_yaml_flattening():
    x = torch.tensor([0.0, 0.25, 1.0])
    assert torch.allclose(inverse_sigmoid(x), O.inverse_sigmoid(x))
    ns = config.flatten_yaml_config({"lr": {"desc": "x", "value": 1e-4}, "backbone": {"value": "video-swin-t"},
                                     "plain": 3}, {"backbone": "video-swin-b", "unset": None})
    assert ns.lr == 1e-4 and ns.backbone == "video-swin-b" and ns.plain == 3 and not hasattr(ns, "unset")


def test_product_package_never_imports_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    pkg = os.path.join(ROOT, "neurips2023_soc_amd")
    pat = re.compile(r"^\s*(from|import)\s+oracle\b|soc_oracle|c_oracle", re.M)
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not pat.search(src), f"{f} references the oracle"
    bench = open(os.path.join(ROOT, "bench.py")).read()
    assert bench.count("from oracle import") == 1   # the cpu_baseline leg only


def test_broadcast_rows_forms():
    """hot_ops._broadcast_rows: how a positional term broadcasts over the flattened rows of x (K7's x_add)."""
    from neurips2023_soc_amd.hot_ops import _broadcast_rows
    K = 16
    pos = torch.randn(5, K)
    x_lead = (3, 5)
    # batch-first: the same [Q,K] table for every frame -> row m uses pos[m % 5]
    base, div, mod = _broadcast_rows(pos[None].expand(3, 5, K), x_lead, K)
    assert (div, mod) == (1, 5) and base.data_ptr() == pos.data_ptr()
    # sequence-first: [Q,1,K] expanded over the frame dim -> row m uses pos[m // 3]
    base, div, mod = _broadcast_rows(pos[:, None].expand(5, 3, K), (5, 3), K)
    assert (div, mod) == (3, 5) and base.data_ptr() == pos.data_ptr()
    # plain contiguous tensor of x's shape
    full = torch.randn(3, 5, K)
    base, div, mod = _broadcast_rows(full, x_lead, K)
    assert (div, mod) == (1, 15) and base.shape == (15, K)
    # a single row broadcast everywhere
    base, div, mod = _broadcast_rows(pos[:1][None].expand(3, 5, K), x_lead, K)
    assert (div, mod) == (1, 1)
    # every row checked against x + add
    x = torch.randn(3, 5, K)
    for add in (pos[None].expand(3, 5, K), full, pos[:1][None].expand(3, 5, K)):
        base, div, mod = _broadcast_rows(add, x_lead, K)
        rows = torch.arange(15)
        assert torch.equal(x.reshape(15, K) + base[(rows // div) % mod], (x + add).reshape(15, K))
    # not of that form: non-contiguous last dim / wrong shape / transposed inner dims
    assert _broadcast_rows(torch.randn(3, 5, 2 * K)[..., ::2], x_lead, K) is None
    assert _broadcast_rows(torch.randn(5, K), x_lead, K) is None
    assert _broadcast_rows(torch.randn(5, 3, K).transpose(0, 1), x_lead, K) is None


def test_fused_linear_uses_library_on_cpu():
    """fused.linear / linear_multi / linear_gelu on CPU tensors: the library path, same numbers as torch."""
    import torch.nn.functional as F
    from neurips2023_soc_amd import fused
    g = torch.Generator().manual_seed(0)
    x, p = torch.randn(7, 32, generator=g), torch.randn(7, 32, generator=g)
    lin = torch.nn.Linear(32, 24)
    assert not fused.is_small(x)          # K7 is GPU-only
    assert torch.equal(fused.linear(x, lin.weight, lin.bias, add=p, relu=True), F.relu(lin(x + p)))
    a, b = fused.linear_multi(x, [(lin.weight, lin.bias, True), (lin.weight, None, False)], p)
    assert torch.equal(a, lin(x + p)) and torch.equal(b, F.linear(x, lin.weight))
    assert torch.equal(fused.linear_gelu(x, lin), F.gelu(lin(x)))


def test_plugin_module_name_and_surface():
    """The reference imports its native op as `MultiScaleDeformableAttention` (functions/ms_deform_attn_func.py:18)
    and the extension exports exactly two functions (src/vision.cpp:13-16).  No CPU path, like the reference's
    (src/cpu/ms_deform_attn_cpu.cpp:26,40): CPU tensors raise."""
    import MultiScaleDeformableAttention as MSDA
    assert sorted(MSDA.__all__) == ["ms_deform_attn_backward", "ms_deform_attn_forward"]
    shapes = torch.tensor([[2, 2]])
    args = (torch.zeros(1, 4, 1, 4), shapes, torch.tensor([0]), torch.zeros(1, 1, 1, 1, 1, 2), torch.zeros(1, 1, 1, 1, 1))
    with pytest.raises(RuntimeError, match="im2col_step"):
        MSDA.ms_deform_attn_forward(*args, 0)
    with pytest.raises(Exception, match="no CPU fallback|MI355X"):
        MSDA.ms_deform_attn_forward(*args, 1)


def test_derived_cache_keys_on_the_tensors_and_dies_with_them():
    """the packed-image caches held strong references (models were never freed), bulk-cleared at a size threshold
    (freeing images whose addresses live captured graphs had baked in) and one keyed on a temporary copy's address.  The
    shared DerivedCache keys on what the tensors are (so per-call views hit), rebuilds after an in-place update, holds weak
    references only and never bulk-clears."""
    import gc

    import torch

    from neurips2023_soc_amd import hot_ops
    c = hot_ops.DerivedCache()
    w, b = torch.nn.Parameter(torch.randn(6, 4)), torch.nn.Parameter(torch.randn(6))
    built = []

    def build():
        built.append(len(built))
        return len(built)
    assert c.get((w[:3], b[:3]), build) == 1 and c.get((w[:3], b[:3]), build) == 1          # a fresh view per call: same entry
    assert c.get((w[3:], b[3:]), build) == 2                                                # other rows: another entry
    wt = w.t()                                                                              # non-contiguous: keyed as it is
    assert c.get((wt,), build) == 3 and c.get((w.t(),), build) == 3
    with torch.no_grad():
        w.mul_(2)
    assert c.get((w[:3], b[:3]), build) == 4                                                # in-place update: rebuilt
    assert c.get((w[:3], None), build, extra=("no bias",)) == 5
    assert len(c) == 4
    del w, wt
    gc.collect()
    assert len(c) == 0                                                                      # freed with the parameter
    # a parameter re-pointed with `p.data = new` keeps its old entry's key reachable for whoever is later
    # allocated at the old address; an entry is only hit while its owner still sits at the keyed address
    p1 = torch.nn.Parameter(torch.randn(8, 4))
    assert c.get((p1,), build) == 6 and c.get((p1,), build) == 6
    old = p1.data
    key_view = old[:]                    # same address, shape, strides, version as the keyed tensor, another owner
    p1.data = torch.randn(8, 4)
    assert c.get((key_view,), build) == 7                                                   # not the stale image
    assert c.get((p1,), build) == 8 and c.get((p1,), build) == 8                            # the re-pointed parameter: rebuilt once


def test_clip_inferencer_group_bookkeeping_with_a_stub_pipeline(monkeypatch):
    """ClipInferencer.submit / drain with launch groups (group = 1 / 2 / 4 / 8), on CPU with a stub pipeline: every clip's result
    comes back exactly once, under its own tag and original size, in submission order, one replay late; a geometry change and
    the end of the stream drain a part-filled group; group = 1 keeps the one-clip behaviour."""
    import torch

    from neurips2023_soc_amd import infer

    class StubPipe:
        """records = the clip id each slot was staged with; replay() returns the previous replay's records (DEPTH 2)"""
        def __init__(self, clips):
            self.CLIPS = clips
            self.slots = [None] * clips
            self.in_head, self.n = None, 0
            self.record = None

        def stage_inputs(self, clip, ids, attn=None, slot=0):
            self.slots[slot] = float(clip.reshape(-1)[0])
            if self.CLIPS > 1:           # the static inputs a group graph keeps: the remainder policy reads the staged clips back from them
                if getattr(self, "clip", None) is None or self.clip.shape[2:] != clip.shape[1:]:
                    self.clip = torch.zeros(clip.shape[0], self.CLIPS, *clip.shape[1:])
                    self.ids = torch.ones(self.CLIPS, ids.numel(), dtype=torch.long)
                    self.attn = torch.ones(self.CLIPS, ids.numel(), dtype=torch.long)
                self.clip[:, slot] = clip
                self.ids[slot] = ids.view(-1)

        def replay(self):
            prev, self.in_head = self.in_head, list(self.slots)
            self.n += 1
            if self.n >= 2:
                self.record = torch.tensor([[v if v is not None else -1.0] for v in prev])
                return self.record if self.CLIPS > 1 else self.record[0]
            return None

        def flush(self):
            if self.n == 0:
                return []
            rec = torch.tensor([[v if v is not None else -1.0] for v in self.in_head])
            self.n, self.in_head = 0, None
            return [rec if self.CLIPS > 1 else rec[0]]

    class Model:
        num_queries = 1

    for group in (1, 2, 3, 4, 8, 10):
        eng = infer.ClipInferencer(Model(), "cpu", use_graphs=True, group=group)
        made = []

        def pipeline(key, eng=eng, group=group, made=made):
            if key not in eng._pipes:
                eng._pipes[key] = StubPipe(group)
                made.append(key)
            return eng._pipes[key]

        monkeypatch.setattr(eng, "_pipeline", pipeline)
        singles = {}
        monkeypatch.setattr(eng, "_single_pipeline", lambda key, singles=singles: singles.setdefault(key, StubPipe(1)))
        monkeypatch.setattr(eng, "_unpack", lambda rec, key, tag, osz: {"tag": tag, "osz": osz, "clip": float(rec.view(-1)[0]), "key": key})
        got = []
        # 7 clips of one geometry, then 3 of another (drains a part-filled group), then the end of the stream
        stream = [(i, (8, 4, 6)) for i in range(7)] + [(100 + i, (8, 6, 6)) for i in range(3)]
        for cid, (T, H, W) in stream:
            clip = torch.full((T, 3, H, W), float(cid))
            got += eng.submit(clip, torch.ones(1, 5, dtype=torch.long), ("tag", cid), (H * 2, W * 2))
        got += eng.drain()
        assert [r["clip"] for r in got] == [float(c) for c, _ in stream], (group, [r["clip"] for r in got])
        assert all(r["tag"] == ("tag", int(r["clip"])) for r in got)
        assert all(r["osz"] == (r["key"][1] * 2, r["key"][2] * 2) for r in got)
        assert len(made) == 2 and eng.drain() == []
        # 7 + 3 clips: full groups, then per geometry a remainder -- at least half a group: one replay with stale slots; fewer:
        # the one-clip pipeline of that geometry
        if group > 1:
            rests = [7 % group, 3 % group]
            assert eng.stats["remainder_singles"] == sum(r for r in rests if 2 * r < group), (group, eng.stats)
            assert eng.stats["stale_slots"] == sum(group - r for r in rests if r and 2 * r >= group), (group, eng.stats)
            assert set(singles) <= set(made)
    import pytest
    with pytest.raises(ValueError):
        infer.ClipInferencer(Model(), "cpu", group=0)


def test_slice_state_gives_views_of_a_sub_group():
    """SOC.slice_state / split_state: clips b0 .. b1 - 1 of a batched head's hand-over state as views (no copies), frames of a
    clip contiguous in the '(b t)' rows; B = 1 passes through."""
    import torch
    from neurips2023_soc_amd.soc import SOC
    B, T, S, C, L = 4, 3, 10, 8, 5
    memory = torch.arange(B * T * S * C, dtype=torch.float32).view(B * T, S, C)
    ratios, mask = torch.rand(B * T, 4, 2), torch.zeros(B * T, S, dtype=torch.bool)
    state = {"ctx": (memory, "shapes", "starts", ratios, mask, False, [(2, 5)]), "feats0": torch.rand(B * T, 6, 7, C),
             "lang_last": torch.rand(L, B, C), "word_pad": torch.zeros(B, L, dtype=torch.bool), "sentence": torch.rand(B, C),
             "B": B, "T": T}
    sub = SOC.slice_state(state, 1, 3)
    assert sub["B"] == 2 and sub["T"] == T
    assert sub["ctx"][0].data_ptr() == memory[T:].data_ptr() and sub["ctx"][0].shape[0] == 2 * T
    assert torch.equal(sub["ctx"][3], ratios[T:3 * T]) and sub["ctx"][1:3] == ("shapes", "starts") and sub["ctx"][5:] == (False, [(2, 5)])
    assert torch.equal(sub["lang_last"], state["lang_last"][:, 1:3]) and torch.equal(sub["sentence"], state["sentence"][1:3])
    assert sub["feats0"].data_ptr() == state["feats0"][T:].data_ptr() and sub["word_pad"].shape == (2, L)
    singles = SOC.split_state(state)
    assert len(singles) == B and all(s["B"] == 1 for s in singles)
    assert torch.equal(singles[3]["ctx"][0], memory[3 * T:]) and torch.equal(singles[0]["lang_last"], state["lang_last"][:, :1])
    one = dict(state, B=1)
    assert SOC.split_state(one) == [one]


@pytest.mark.parametrize("clips", [1, 3])
def test_pipelined_runner_replay_order(clips):
    """PipelinedClipGraph and a launch group drive their captured graphs alike: head only after a flush, then steady graphs 1, 0, 1 ...
    (graph k fills sb[k]), and a flush drains the state the last head wrote.  No GPU: the graphs are stubs that log their name."""
    from neurips2023_soc_amd import graph_runner as G
    cls = G.PipelinedClipGraph if clips == 1 else G.group_pipeline_class(clips)
    log = []

    class Stub:
        def __init__(self, name):
            self.name = name

        def replay(self):
            log.append(self.name)

    g = object.__new__(cls)
    g.first, g.steady, g.drain = Stub("first"), [Stub("steady0"), Stub("steady1")], [Stub("drain0"), Stub("drain1")]
    g._n, g.record = 0, torch.zeros(4) if clips == 1 else torch.zeros(clips, 4)
    assert g.CLIPS == clips and g.DEPTH == 2
    assert [g.replay() for _ in range(3)] == [None, g.record, g.record]
    flushed = [g.flush()]
    assert g.replay() is None
    flushed += [g.flush(), g.flush()]
    assert log == ["first", "steady1", "steady0", "drain0", "first", "drain0"]
    assert [len(f) for f in flushed] == [1, 1, 0]
    assert all(torch.equal(f[0], g.record) and f[0].data_ptr() != g.record.data_ptr() for f in flushed[:2])


@pytest.mark.parametrize("clips", [1, 3])
def test_runner_static_inputs_and_staging(clips, monkeypatch):
    """The one allocation rule and the one stage_inputs of every graph runner, on CPU buffers: layouts per clip count, accepted
    input shapes, and the attention mask of a slot going back to ones when ids are staged without one -- per slot."""
    from neurips2023_soc_amd import graph_runner as G

    class Model:
        num_queries = 2

    fills, fill_ = [], torch.Tensor.fill_
    monkeypatch.setattr(torch.Tensor, "fill_", lambda t, v: fills.append(v) or fill_(t, v))
    T, H, W, L = 2, 8, 8, 5
    g = object.__new__(G.ClipGraph if clips == 1 else G.group_pipeline_class(clips))
    g._allocate(Model(), T, H, W, L, "cpu")
    R = g.record.shape[-1]
    assert g.clip.shape == (T, clips, 3, H, W) and g.pad.shape == (T, clips, H, W) and g.pad.dtype == torch.bool
    assert g.ids.shape == g.attn.shape == (clips, L) and len(g.targets) == T
    flat = g.clip.transpose(0, 1).flatten(0, 1)                  # the backbone's '(b t)' flatten: a view for every clip count
    assert flat.data_ptr() == g.clip.data_ptr() and flat.is_contiguous()
    if clips == 1:
        assert g.clip.is_contiguous() and g.record.dim() == 1 and g.record[None].shape == (1, R)
    else:
        assert g.record.shape == (clips, R)
    ids, mask = torch.arange(2, 2 + L), torch.tensor([1, 1, 1, 0, 0])
    clip = torch.randn(T, 3, H, W)
    if clips == 1:
        g.stage_inputs(clip, ids[None], mask[None])
        assert torch.equal(g.clip[:, 0], clip) and torch.equal(g.ids[0], ids) and torch.equal(g.attn[0], mask)
        g.stage_inputs(2 * clip[:, None], ids[None] + 1)          # [T,1,3,H,W]; no mask: ones again
        assert torch.equal(g.clip[:, 0], 2 * clip) and torch.equal(g.ids[0], ids + 1) and bool((g.attn == 1).all())
        g.stage_inputs(clip, ids[None], mask[None])
        g.stage_inputs(3 * clip)                                  # ids=None: ids and mask stay as staged
        assert torch.equal(g.clip[:, 0], 3 * clip) and torch.equal(g.ids[0], ids) and torch.equal(g.attn[0], mask)
    else:
        g.stage_inputs(clip, ids[None], mask[None], slot=1)       # ids as [1,L] ...
        g.stage_inputs(2 * clip, ids + 1, mask.flip(0), slot=2)   # ... or [L]
        assert torch.equal(g.clip[:, 1], clip) and torch.equal(g.clip[:, 2], 2 * clip) and not g.clip[:, 0].any()
        assert torch.equal(g.attn[1], mask) and torch.equal(g.attn[2], mask.flip(0))
        g.stage_inputs(3 * clip, ids + 2, slot=1)                 # slot 1 back to ones, slot 2 as staged
        assert torch.equal(g.clip[:, 1], 3 * clip) and torch.equal(g.ids[1], ids + 2) and torch.equal(g.ids[2], ids + 1)
        assert bool((g.attn[1] == 1).all()) and torch.equal(g.attn[2], mask.flip(0))
        assert bool((g.ids[0] == 1).all()) and bool((g.attn[0] == 1).all())      # never staged
    # staging adds no launch: the mask was refilled once above, for the slot that held another one, and an unmasked slot never is
    assert len(fills) == 1
    g.stage_inputs(clip, ids, mask, slot=clips - 1)
    for _ in range(2):
        g.stage_inputs(clip, ids, slot=clips - 1)
        g.stage_inputs(clip, ids, slot=0)
    assert len(fills) == 2
