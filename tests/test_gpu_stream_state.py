"""-m gpu: LONG streams through one model object -- cached constants under live hipGraphs, and weight reloads.

The dataset drivers push hundreds of clips of changing geometry through one ClipInferencer, which keeps up to four captured graphs
per kind while the model's host-side caches (the transformer's _unpadded_cache, the DerivedCache instances, the FPN's _tap_cache,
the K3 workspaces ...) evict and rebuild entries whose device tensors those graphs have baked in by address.  These tests run such
streams and check every result against the CPU oracle (oracle.soc_oracle.soc_forward on the same synthetic weights, clip and token
ids: independent of the code under test).

Bounds against the oracle: mask logits 1.2e-3 (the 1e-3 GPU-to-reference bound of test_gpu_forward.py plus the 2e-4
oracle-to-reference bound of test_oracle_odd_geometries), pred_cls 1e-4, pred_boxes 1e-5.  Graph against eager on one model: 1e-4
(test_clip_inferencer_pads_expressions_for_graph_reuse); two runs of one model: 5e-4 (test_forward_repeatable_...).

The selected query must equal the oracle's.  Every case's clip seed was picked on the CPU, with the oracle alone, so that the
oracle's own best and second-best trajectory scores are at least GAP = 1e-2 apart, and the oracle asserts it again here for every
case (no case is skipped).  The gap is measured on the LOGIT scale, logit(s_best) - logit(s_second) with s_q = mean_t
sigmoid(pred_cls[t, q]) (what select_trajectory ranks): with the synthetic weights the sigmoid scores of all 20 queries lie within
1e-2 of each other (seed 2023: 0.015 .. 0.04) or within 3e-4 (seed 7: all below 1e-3), so no clip has a gap of 1e-2 between two of
them (0 of 80 scanned), while pred_cls is bounded at 1e-4 on the logit scale.  If every logit moves by at most 1e-4, logit(s_q)
moves by at most 1e-4 (d/dx logit(mean_t sigmoid(x_t + x)) = mean_t s_t (1 - s_t) / (s (1 - s)) <= 1, p (1 - p) being concave), so
a gap of 1e-2 is 50 times what the pred_cls bound lets two scores approach each other by.

Liveness first: the tests that revisit a live graph after the constants cache has turned over record weak references to what each
capture was handed (a wrapper around _unpadded_constants) and assert, BEFORE the replay, that those tensors are still allocated.  A
graph whose constants have died is never replayed: the test fails at that assertion instead of reading freed memory.
"""
import math
import weakref

import numpy as np
import pytest
import torch

import neurips2023_soc_amd as S
from neurips2023_soc_amd import fused, graph_runner, hot_ops, postprocessing as P, weights as W
from neurips2023_soc_amd.infer import ClipInferencer
from oracle import soc_oracle as O

pytestmark = pytest.mark.gpu

GAP = 1e-2
MASKS, CLS, BOXES = 1.2e-3, 1e-4, 1e-5
GRAPH_VS_EAGER, REPEAT = 1e-4, 5e-4
L = 6

# (T, H, W, clip seeds): 18 distinct geometries, sizes that pad at every stage among them (36 -> 9 -> 5 -> 3 -> 2 rows); every
# (T, ceil(H / 8), ceil(W / 8)) is distinct, so each is its own key of the constants cache.  Seeds: see the module docstring.
CASES_A = [
    (1, 32, 32, [400]),
    (1, 36, 52, [410]),
    (1, 40, 64, [420]),
    (1, 44, 60, [430]),
    (1, 48, 40, [440]),
    (1, 56, 36, [450]),
    (2, 32, 48, [460]),
    (2, 36, 44, [470]),
    (2, 40, 32, [482]),
    (2, 52, 64, [490]),
    (2, 60, 36, [500]),
    (2, 64, 56, [512]),
    (3, 32, 40, [521]),
    (3, 44, 36, [531]),
    (3, 48, 64, [540, 541]),
    (3, 52, 52, [550, 551]),
    (3, 56, 48, [560, 561]),
    (3, 64, 32, [570]),
]
LIVE_B = (2, 48, 48, [600, 601])            # the live graph of 2b, two clips
# ten geometries, five clips each + one more for the return visit
CASES_C = [
    (1, 32, 48, [700, 701, 702, 706, 707, 708]),
    (2, 36, 36, [722, 723, 724, 725, 728, 729]),
    (3, 40, 40, [740, 742, 743, 744, 745, 746]),
    (1, 52, 44, [761, 762, 763, 764, 765, 766]),
    (2, 48, 56, [780, 782, 783, 784, 785, 786]),
    (3, 36, 60, [800, 801, 802, 803, 804, 805]),
    (1, 64, 64, [820, 821, 822, 823, 824, 825]),
    (2, 56, 40, [840, 843, 845, 847, 848, 853]),
    (3, 32, 32, [860, 862, 866, 870, 872, 873]),
    (2, 44, 60, [882, 885, 886, 887, 888, 889]),
]
E_GEOM, E_2023, E_7 = (2, 48, 64), [900, 901, 902], [922, 923, 924]        # clip seeds under the seed-2023 / seed-7 weights
# weight reload, eager: the tiny golden geometry (K23, K12) and the BASELINE geometry (K20, K24, K23, the stacked K20 pair)
D_TINY, D_FULL = {"7": 940, "7e": 940}, {"7": 960, "7e": 960}        # clip seeds under seed 7 / seed 7 with the edits below
D_GEOMS = {"tiny": (3, 250, 300, 10), "full": (8, 360, 640, 10)}
# one parameter behind each cache family, edited with p.copy_() under no_grad
EDITED = {
    "k20": "vlf.multihead_attn.out_proj.weight",
    "k24": "backbone.0.body.layers.2.blocks.0.attn.qkv.weight",
    "k23": "backbone.0.body.layers.0.blocks.0.mlp.fc2.weight",
    "stacked": "transformer.encoder.layers.0.self_attn.attention_weights.weight",
    "fpn": "spatial_decoder.out_lay.weight",
    "level_embed": "transformer.level_embed",
}


def edited_value(t):
    """what p.copy_() writes in 2d: the tensor scaled by a ramp from 0.25 to 1 over its elements (not a uniform factor, which a
    normalisation behind the layer could cancel)"""
    return t * torch.linspace(0.25, 1.0, t.numel()).view(t.shape)


def maxdiff(a, b):
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max())


def build(sd):
    assert torch.cuda.is_available()
    model, _, _ = S.build_model(S.default_args(text_encoder_random_init=True))
    model.load_state_dict(sd, strict=False)
    return model.cuda().eval()


@pytest.fixture(scope="module")
def sd7(ref_shapes):
    shapes = {k: v[0] for k, v in ref_shapes("t").items() if v[1].startswith("float")}
    return W.synthetic_state_dict(shapes, seed=7)


@pytest.fixture()
def model(synthetic_sd):
    return build(synthetic_sd)


class Oracle:
    """Memo of oracle forwards per (weights tag, clip seed, geometry); asserts the selection gap of every case."""

    def __init__(self):
        self.text, self.memo = {}, {}

    def __call__(self, tag, sd, seed, T, H, Wd, n_tokens=L):
        key = (tag, seed, T, H, Wd, n_tokens)
        if key not in self.memo:
            if tag not in self.text:
                self.text[tag] = O.build_text_encoder(sd)
            clip, ids = W.synthetic_clip(seed, T, H, Wd), W.synthetic_token_ids(seed, n_tokens)
            ref = O.soc_forward(sd, clip, ids, torch.ones_like(ids), (H, Wd), text_encoder=self.text[tag])
            s = ref["pred_cls"][:, 0].sigmoid().mean(0).max(-1)[0].double()
            top = s.topk(2).values
            gap = math.log(float(top[0]) / (1 - float(top[0]))) - math.log(float(top[1]) / (1 - float(top[1])))
            assert gap > GAP, f"oracle selection gap {gap:.2e} of case {key}: pick another seed"
            self.memo[key] = {"pred_masks": ref["pred_masks"], "pred_cls": ref["pred_cls"], "pred_boxes": ref["pred_boxes"],
                              "query": int(s.argmax()), "gap": gap}
        return self.memo[key]


ORACLE = Oracle()


def inputs(seed, T, H, Wd, n_tokens=L):
    return W.synthetic_clip(seed, T, H, Wd).cuda(), W.synthetic_token_ids(seed, n_tokens).cuda()


def check_full(out, ref, what):
    """A forward's output dict against the oracle's: all mask logits, class logits, boxes, the selected query.  -> mask logits (CPU)."""
    torch.cuda.synchronize()
    masks = out["pred_masks"].detach().cpu().clone()
    d = (maxdiff(masks, ref["pred_masks"]), maxdiff(out["pred_cls"], ref["pred_cls"]), maxdiff(out["pred_boxes"], ref["pred_boxes"]))
    idx, _ = P.select_trajectory(out)
    print(f"{what}: masks {d[0]:.2e} (of {float(ref['pred_masks'].abs().max()):.1f}) cls {d[1]:.2e} boxes {d[2]:.2e} "
          f"query {int(idx)} / {ref['query']} (gap {ref['gap']:.2e})")
    assert d[0] < MASKS and d[1] < CLS and d[2] < BOXES, (what, d)
    assert int(idx) == ref["query"], what
    return masks


def check_result(res, ref, what):
    """A ClipInferencer result (selected query, its mask logits, the class logits) against the oracle's.  -> its mask logits (CPU)."""
    q = int(res["query"])
    masks = res["mask_logits"].detach().cpu().clone()
    d = (maxdiff(masks, ref["pred_masks"][:, 0, ref["query"]]), maxdiff(res["pred_cls"], ref["pred_cls"][:, 0, :, 0]))
    print(f"{what}: masks {d[0]:.2e} cls {d[1]:.2e} query {q} / {ref['query']} (gap {ref['gap']:.2e})")
    assert q == ref["query"], what
    assert d[0] < MASKS and d[1] < CLS, (what, d)
    return masks


class Constants:
    """Wrapper around DeformableTransformer._unpadded_constants: which keys were asked for, and weak references to the tensors every
    graph runner was handed during its warm-up and capture."""

    def __init__(self, model, monkeypatch):
        self.log, self.owner = [], {}
        tr = model.transformer
        real = tr._unpadded_constants

        def recording(shapes, n, pos_embeds, device):
            const = real(shapes, n, pos_embeds, device)
            self.log.append((tuple(shapes), n, [weakref.ref(v) for v in const.values() if v is not None]))
            return const

        monkeypatch.setattr(tr, "_unpadded_constants", recording)

    def keys(self):
        """distinct cache keys seen so far (NOT the current length of the cache)"""
        return len({(s, n) for s, n, _ in self.log})

    def call(self, engine, fn, *args, **kwargs):
        """fn(*args) on `engine`; the runners it created are credited with the constants handed out meanwhile"""
        since = len(self.log)
        result = fn(*args, **kwargs)
        for kind in (engine._graphs, engine._pipes, engine._singles):
            for r in kind.values():
                known = self.owner.get(id(r))
                if known is not None and known[0]() is r:
                    continue
                first_level = (-(-(-(-r.H // 4)) // 2), -(-(-(-r.W // 4)) // 2))
                mine = [refs for s, n, refs in self.log[since:] if n == r.CLIPS * r.T and s[0] == first_level]
                assert mine, "a runner was captured without asking for its constants"
                self.owner[id(r)] = (weakref.ref(r), [x for refs in mine for x in refs])
        return result

    def alive(self, runner):
        known = self.owner[id(runner)]
        assert known[0]() is runner
        return len(known[1]) >= 4 and all(x() is not None for x in known[1])


def test_geometry_churn_under_live_clip_graphs(model, synthetic_sd, monkeypatch):
    """2a.  18 geometries captured in order through ClipInferencer(max_graphs=4): the 18th key of the constants cache arrives while
    graphs 15-17 are still held.  Then back through those three, each with a clip it has not seen and with its first clip again."""
    const = Constants(model, monkeypatch)
    engine = ClipInferencer(model, "cuda", use_graphs=True, max_graphs=4)
    first = {}
    for i, (T, H, Wd, seeds) in enumerate(CASES_A):
        out, _ = const.call(engine, engine.forward_clip, *inputs(seeds[0], T, H, Wd))
        first[i] = check_full(out, ORACLE("2023", synthetic_sd, seeds[0], T, H, Wd), f"capture {i} {(T, H, Wd)}")
        assert len(engine._graphs) <= 4
    assert len(CASES_A) == 18 and const.keys() >= 18, const.keys()
    assert list(engine._graphs) == [(T, H, Wd, L) for T, H, Wd, _ in CASES_A[14:]]
    for i in (14, 15, 16):
        T, H, Wd, seeds = CASES_A[i]
        runner = engine._graphs[(T, H, Wd, L)]
        for seed in (seeds[1], seeds[0]):
            assert const.alive(runner), f"the constants graph {i} was captured with have been freed: not replaying it"
            calls = len(const.log)
            out, _ = engine.forward_clip(*inputs(seed, T, H, Wd))
            assert engine._graphs[(T, H, Wd, L)] is runner and len(const.log) == calls          # a replay, not a new capture
            masks = check_full(out, ORACLE("2023", synthetic_sd, seed, T, H, Wd), f"revisit {i} seed {seed}")
        assert maxdiff(masks, first[i]) < REPEAT
        assert len(engine._graphs) <= 4


def test_eager_traffic_beside_one_live_graph(model, synthetic_sd, monkeypatch):
    """2b.  One captured geometry; 18 eager forwards of 18 other geometries add 18 new keys to the constants cache; the live graph
    is replayed after every third of them, alternating between two clips."""
    const = Constants(model, monkeypatch)
    graphs = ClipInferencer(model, "cuda", use_graphs=True)
    eager = ClipInferencer(model, "cuda", use_graphs=False)
    T0, H0, W0, live_seeds = LIVE_B
    assert (T0, H0, W0) not in [c[:3] for c in CASES_A]
    out, _ = const.call(graphs, graphs.forward_clip, *inputs(live_seeds[0], T0, H0, W0))
    first = check_full(out, ORACLE("2023", synthetic_sd, live_seeds[0], T0, H0, W0), "capture")
    runner = graphs._graphs[(T0, H0, W0, L)]
    ref_eager = eager.forward_clip(*inputs(live_seeds[0], T0, H0, W0))[0]
    assert maxdiff(ref_eager["pred_masks"], first) < GRAPH_VS_EAGER
    replays = 0
    for j, (T, H, Wd, seeds) in enumerate(CASES_A):
        out, _ = eager.forward_clip(*inputs(seeds[0], T, H, Wd))
        check_full(out, ORACLE("2023", synthetic_sd, seeds[0], T, H, Wd), f"eager {j} {(T, H, Wd)}")
        if j % 3 == 2:
            assert const.alive(runner), f"after {const.keys()} keys the live graph's constants have been freed: not replaying it"
            calls = len(const.log)
            seed = live_seeds[(replays + 1) % 2]
            out, _ = graphs.forward_clip(*inputs(seed, T0, H0, W0))
            assert graphs._graphs[(T0, H0, W0, L)] is runner and len(const.log) == calls
            masks = check_full(out, ORACLE("2023", synthetic_sd, seed, T0, H0, W0), f"replay after eager {j}")
            if seed == live_seeds[0]:
                assert maxdiff(masks, first) < REPEAT
            replays += 1
    assert const.keys() >= 19 and replays == 6, (const.keys(), replays)       # the last replay came after the 18th new key


def test_streaming_groups_through_changing_geometries(model, synthetic_sd, monkeypatch):
    """2c.  ClipInferencer(group=4), submit() / drain(): ten geometries, five clips each -- one full group and a remainder of one that
    leaves through the one-clip pipeline, so every geometry adds the n = 4T and the n = T key and captures a group pipeline and a
    one-clip pipeline; every other geometry also runs one clip through __call__ (a ClipGraph), so that all three graph dictionaries
    evict.  Every clip comes back exactly once, under its own tag, with its own oracle result.  Then back to the three most recent
    geometries, whose runners are still held."""
    const = Constants(model, monkeypatch)
    engine = ClipInferencer(model, "cuda", use_graphs=True, group=4)
    got = {}

    def collect(results):
        for res in results:
            assert res["tag"] not in got, res["tag"]
            gi, ci = res["tag"][:2]
            T, H, Wd, seeds = CASES_C[gi]
            got[res["tag"]] = check_result(res, ORACLE("2023", synthetic_sd, seeds[ci], T, H, Wd), f"tag {res['tag']}")

    def stream(gi, order, mark=()):
        T, H, Wd, seeds = CASES_C[gi]
        for ci in order:
            collect(const.call(engine, engine.submit, *inputs(seeds[ci], T, H, Wd), (gi, ci) + mark))

    for gi, (T, H, Wd, seeds) in enumerate(CASES_C):
        stream(gi, range(5))                  # the first submit of a new geometry drains the one before it
        if gi % 2:
            collect(const.call(engine, engine.drain))
            res = const.call(engine, engine, *inputs(seeds[0], T, H, Wd))
            masks = check_result(res, ORACLE("2023", synthetic_sd, seeds[0], T, H, Wd), f"ClipGraph of geometry {gi}")
            assert maxdiff(masks, got[(gi, 0)]) < GRAPH_VS_EAGER
        for kind in (engine._graphs, engine._pipes, engine._singles):
            assert len(kind) <= 4
    collect(const.call(engine, engine.drain))
    assert sorted(got) == [(gi, ci) for gi in range(len(CASES_C)) for ci in range(5)] and len(CASES_C) >= 10
    assert const.keys() >= 20, const.keys()                                   # n = 4T and n = T of ten geometries: past the 18th key
    assert engine.stats["remainder_singles"] == len(CASES_C) and engine.stats["group_replays"] == len(CASES_C)
    held = [(T, H, Wd, L) for T, H, Wd, _ in CASES_C[-4:]]
    assert list(engine._pipes) == held and list(engine._singles) == held and len(engine._graphs) == 4
    for gi in (len(CASES_C) - 3, len(CASES_C) - 2, len(CASES_C) - 1):
        T, H, Wd, seeds = CASES_C[gi]
        key = (T, H, Wd, L)
        pipe, single = engine._pipes[key], engine._singles[key]
        assert const.alive(pipe) and const.alive(single), f"constants of the pipelines of geometry {gi} have been freed: not replaying"
        calls = len(const.log)
        stream(gi, (5, 3, 1, 4, 2), mark=("again",))          # a clip it has not seen, and other slots for the rest
        collect(engine.drain())
        assert engine._pipes[key] is pipe and engine._singles[key] is single and len(const.log) == calls
        for ci in (1, 2, 3, 4):
            assert maxdiff(got[(gi, ci, "again")], got[(gi, ci)]) < REPEAT
    assert len(got) == 50 + 15


def run_geom(model, tag, sd, seed, name):
    T, H, Wd, n_tokens = D_GEOMS[name]
    out, _ = ClipInferencer(model, "cuda", use_graphs=False).forward_clip(*inputs(seed, T, H, Wd, n_tokens))
    return check_full(out, ORACLE(tag, sd, seed, T, H, Wd, n_tokens), f"weights {tag} {name}")


def behind(cache, p):
    """is parameter `p` one of the tensors an entry of this DerivedCache is keyed on"""
    return any(isinstance(e, tuple) and len(e) == 6 and e[0] == p.data_ptr() for key in cache._d for e in key)


def test_weight_reload_eager(model, synthetic_sd, sd7, golden):
    """2d.  Fill every cache under seed 2023 (tiny + BASELINE geometry), load seed 7 in place: the results are the oracle's at seed 7
    and those of a model that only ever saw seed 7.  Then p.copy_() on one parameter behind each cache family, a .cpu() / .cuda()
    round trip, and seed 2023 back against the reference's golden."""
    from tests.test_gpu_forward import FLIP_WINDOW, run_cfg
    params = dict(model.named_parameters())
    g_tiny, g_full = golden("tiny_forward.npz"), golden("full_forward.npz")
    assert tuple(int(v) for v in g_tiny["cfg"][1:]) == D_GEOMS["tiny"] and tuple(int(v) for v in g_full["cfg"][1:]) == D_GEOMS["full"]

    def golden_checks():
        out = run_cfg(model, g_tiny["cfg"])
        assert maxdiff(out["pred_masks"], g_tiny["pred_masks"]) < 1e-3
        flip = (out["pred_masks"].cpu().numpy() > 0) != (g_tiny["pred_masks"] > 0)
        assert flip.sum() <= 2 and (not flip.any() or np.abs(g_tiny["pred_masks"][flip]).max() < FLIP_WINDOW)
        assert maxdiff(out["pred_cls"], g_tiny["pred_cls"]) < 1e-4
        assert maxdiff(out["pred_boxes"], g_tiny["pred_boxes"]) < 1e-5
        assert maxdiff(out["pred_logit"], g_tiny["pred_logit"]) < 1e-4
        assert maxdiff(out["text_sentence_feature"], g_tiny["text_sentence_feature"]) < 1e-4
        out = run_cfg(model, g_full["cfg"])
        idx, masks = P.select_trajectory(out)
        assert int(idx) == int(g_full["selected_query"])
        assert maxdiff(masks, g_full["selected_masks"]) < 1e-3
        assert maxdiff(out["pred_cls"], g_full["pred_cls"]) < 1e-4
        assert maxdiff(out["pred_boxes"], g_full["pred_boxes"]) < 1e-5

    golden_checks()
    # the run above went through every cache family, and the parameters edited below sit behind them
    assert behind(hot_ops._split_cache, params[EDITED["k20"]])
    assert behind(hot_ops._xs_cache, params[EDITED["k24"]])
    assert behind(hot_ops._mlp_cache, params[EDITED["k23"]])
    assert behind(fused._stack_cache, params[EDITED["stacked"]])
    assert len(model.spatial_decoder._tap_cache) >= 4 and len(model.transformer._unpadded_cache) >= 2

    model.load_state_dict(sd7, strict=False)
    fresh = build(sd7)
    before = {}
    for name, seeds in (("tiny", D_TINY), ("full", D_FULL)):
        before[name] = run_geom(model, "7", sd7, seeds["7"], name)
        T, H, Wd, n_tokens = D_GEOMS[name]
        other = ClipInferencer(fresh, "cuda", use_graphs=False).forward_clip(*inputs(seeds["7"], T, H, Wd, n_tokens))[0]
        assert maxdiff(other["pred_masks"], before[name]) < REPEAT, name
    del fresh

    # p.copy_() under no_grad, one family at a time: each edit must be SEEN (the BASELINE geometry's output moves by far more than
    # the run-to-run noise), and with all six in place the results are the oracle's for the edited weights
    sd7e = dict(sd7)
    T, H, Wd, n_tokens = D_GEOMS["full"]
    probe = inputs(D_FULL["7e"], T, H, Wd, n_tokens)
    eager = ClipInferencer(model, "cuda", use_graphs=False)
    last = eager.forward_clip(*probe)[0]["pred_masks"].cpu().clone()
    for family, name in EDITED.items():
        assert "bbox_embed" not in name
        sd7e[name] = edited_value(sd7[name])
        with torch.no_grad():
            params[name].copy_(sd7e[name])
        now = eager.forward_clip(*probe)[0]["pred_masks"].cpu().clone()
        moved = maxdiff(now, last)
        print(f"edit {family} ({name}): output moved by {moved:.2e}")
        assert moved > 10 * REPEAT, (family, moved)
        last = now
    edited = {name: run_geom(model, "7e", sd7e, seeds["7e"], name) for name, seeds in (("tiny", D_TINY), ("full", D_FULL))}

    model.cpu()
    model.cuda()
    for name, seeds in (("tiny", D_TINY), ("full", D_FULL)):
        assert maxdiff(run_geom(model, "7e", sd7e, seeds["7e"], name), edited[name]) < REPEAT, name

    model.load_state_dict(synthetic_sd, strict=False)
    golden_checks()


def test_weight_reload_with_graphs_alive(model, synthetic_sd, sd7, monkeypatch):
    """2e.  After load_state_dict on a model whose ClipInferencer holds graphs, the same inferencer's next results are the new weights'
    (checked against the oracle); a runner captured under the old weights is not replayed (guarded BEFORE the replay: a packed weight
    image it was captured with may have been rebuilt meanwhile)."""
    T, H, Wd = E_GEOM
    engine = ClipInferencer(model, "cuda", use_graphs=True)

    def stream(tag, sd, seeds):
        seen = []
        for s in seeds:
            for res in engine.submit(*inputs(s, T, H, Wd), s):
                check_result(res, ORACLE(tag, sd, res["tag"], T, H, Wd), f"weights {tag}: stream, clip {res['tag']}")
                seen.append(res["tag"])
        for res in engine.drain():
            check_result(res, ORACLE(tag, sd, res["tag"], T, H, Wd), f"weights {tag}: stream, clip {res['tag']}")
            seen.append(res["tag"])
        assert seen == list(seeds)

    out, _ = engine.forward_clip(*inputs(E_2023[0], T, H, Wd))
    check_full(out, ORACLE("2023", synthetic_sd, E_2023[0], T, H, Wd), "weights 2023: ClipGraph")
    stream("2023", synthetic_sd, E_2023)
    old = list(engine._graphs.values()) + list(engine._pipes.values())
    assert len(old) == 2

    model.load_state_dict(sd7, strict=False)

    def guarded(real):
        def replay(self, *args, **kwargs):
            assert not any(self is r for r in old), "replaying a graph that was captured under the old weights"
            return real(self, *args, **kwargs)
        return replay

    for cls in (graph_runner.ClipGraph, graph_runner.PipelinedClipGraph, graph_runner.TwoStreamClipGraph):
        monkeypatch.setattr(cls, "replay", guarded(cls.replay))
    out, _ = engine.forward_clip(*inputs(E_7[0], T, H, Wd))
    check_full(out, ORACLE("7", sd7, E_7[0], T, H, Wd), "weights 7: ClipGraph")
    stream("7", sd7, E_7)
    assert len(engine._graphs) == 1 and len(engine._pipes) == 1
    assert not any(r is o for r in list(engine._graphs.values()) + list(engine._pipes.values()) for o in old)
    # and a second load: back to seed 2023
    old += list(engine._graphs.values()) + list(engine._pipes.values())
    model.load_state_dict(synthetic_sd, strict=False)
    stream("2023", synthetic_sd, E_2023[::-1])
    out, _ = engine.forward_clip(*inputs(E_2023[1], T, H, Wd))
    check_full(out, ORACLE("2023", synthetic_sd, E_2023[1], T, H, Wd), "weights 2023 again: ClipGraph")
