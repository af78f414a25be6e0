"""CPU (-m "not gpu"): a LONG stream of changing geometries through ONE model object, and the lifetime contract of the host-side
caches of device tensors (derived_cache.keep_alive / hold).

The dataset drivers push hundreds of clips of changing geometry through one model whose caches -- the transformer's
_unpadded_cache and _shape_cache, Joiner._pos_cache, the FPN's _tap_cache, the DerivedCache instances -- hand out tensors that a
captured hipGraph bakes in by address.  The contract: what is handed out inside a keep-alive scope (a graph runner opens one around
its warm-up and capture) stays allocated while the scope's holder lives, whatever the cache does with its entry afterwards; without
a holder the caches stay bounded.  The model runs on the CPU with the oracle's kernel-boundary functions patched in (as in
test_host_plumbing.py); the reference is the standalone oracle forward of each geometry.
"""
import contextlib
import gc
import weakref

import pytest
import torch

import neurips2023_soc_amd as S
from neurips2023_soc_amd import derived_cache as DC, weights as W
from oracle import soc_oracle as O
from tests.test_host_plumbing import maxdiff, oracle_kernels  # noqa: F401  (fixture: the same monkeypatch list)

# 19 distinct unpadded geometries (T, H, W): 18 fill and overflow the constants cache (bound: 17 entries), the 19th follows the
# drop.  H, W in {32, 40, 48} give the level shapes (4,2,1) / (5,3,2) / (6,3,2): every (T, H, W) here is its own cache key.
GEOMETRIES = [(T, H, Wd) for T in (1, 2) for H in (32, 40, 48) for Wd in (32, 40, 48)] + [(3, 32, 32)]
L = 6
BOUND = 17          # entries the constants cache may hold with nobody holding on to them


@pytest.fixture(scope="module")
def cpu_model(synthetic_sd):
    model, _, _ = S.build_model(S.default_args(text_encoder_random_init=True, device="cpu"))
    model.load_state_dict(synthetic_sd, strict=False)
    return model.eval()


def inputs(i, geom):
    T, H, Wd = geom
    return W.synthetic_clip(300 + i, T, H, Wd), W.synthetic_token_ids(300 + i, L)


def run(model, clip, ids):
    T, _, H, Wd = clip.shape
    samples = S.nested_tensor_from_videos_list([clip])
    assert samples.unpadded
    targets = [[{"size": torch.tensor([H, Wd])}] for _ in range(T)]
    with torch.no_grad():
        return model(samples, None, {"input_ids": ids, "attention_mask": torch.ones_like(ids)}, targets)


def scope(holder):
    """derived_cache.keep_alive(holder); a tree without the scope has nothing to open, and the liveness assertion fails there."""
    return DC.keep_alive(holder) if hasattr(DC, "keep_alive") else contextlib.nullcontext()


def test_nineteen_geometries_through_one_model(cpu_model, oracle_kernels, synthetic_sd, monkeypatch):  # noqa: F811
    tr = cpu_model.transformer
    tr.__dict__.pop("_unpadded_cache", None)
    text_encoder = O.build_text_encoder(synthetic_sd)
    handed = []                      # per call: (cache key fields that name the geometry, weak references to the tensors handed out)
    real = tr._unpadded_constants

    def recording(shapes, n, pos_embeds, device):
        const = real(shapes, n, pos_embeds, device)
        handed.append(((shapes, n), [weakref.ref(v) for v in const.values() if v is not None]))
        return const

    monkeypatch.setattr(tr, "_unpadded_constants", recording)
    assert GEOMETRIES[0] not in GEOMETRIES[1:] and len(set(GEOMETRIES)) == len(GEOMETRIES) >= 19

    holder, first = [], None
    for i, geom in enumerate(GEOMETRIES + [GEOMETRIES[0]]):
        revisit = i == len(GEOMETRIES)
        clip, ids = inputs(0 if revisit else i, geom)
        if i == 0:
            with scope(holder):      # what a graph runner does around its warm-up and capture
                out = run(cpu_model, clip, ids)
            held = handed[-1][1]
            assert len(held) >= 4 and all(r() is not None for r in held)
        else:
            out = run(cpu_model, clip, ids)
        out = {k: out[k].clone() for k in ("pred_masks", "pred_cls", "pred_boxes")}
        ref = O.soc_forward(synthetic_sd, clip, ids, torch.ones_like(ids), geom[1:], text_encoder=text_encoder)
        d = {k: maxdiff(out[k], ref[k]) for k in out}
        print(i, geom, {k: f"{v:.2e}" for k, v in d.items()}, "cache entries", len(tr._unpadded_cache))
        assert d["pred_masks"] < 1e-3 and d["pred_cls"] < 1e-4 and d["pred_boxes"] < 1e-5, (geom, d)
        assert len(tr._unpadded_cache) <= BOUND, "the constants cache is not bounded"
        if i == 0:
            first = out
        keys = len({k for k, _ in handed})
        if keys >= 18:
            # the keep-alive assertion: the 18th distinct key has made the cache drop the first geometry's entry, and what was
            # handed out inside the scope is still allocated because the scope's holder has it
            assert all(r() is not None for r in held), \
                f"after {keys} distinct keys the constants handed out inside the keep-alive scope have been freed"
        if revisit:
            for k in out:            # same weights, same inputs, rebuilt constants: the same arithmetic
                assert torch.equal(out[k], first[k]), k
    assert len({k for k, _ in handed}) == len(GEOMETRIES)
    # ... and releasing the holder (evicting the runner) releases them: the cache itself dropped its entry at the 18th key
    del holder[:]
    gc.collect()
    assert all(r() is None for r in held), "the constants cache still pins an entry it had dropped"


def test_every_geometry_cache_hands_its_values_to_the_scope(cpu_model, oracle_kernels):  # noqa: F811
    """One forward inside a scope: the holder receives what _unpadded_cache, _shape_cache and _pos_cache handed out (by identity)."""
    tr, joiner = cpu_model.transformer, cpu_model.backbone
    clip, ids = inputs(0, GEOMETRIES[0])
    holder = []
    with DC.keep_alive(holder):
        run(cpu_model, clip, ids)
    got = {id(v) for v in holder}
    n = clip.shape[0]
    const = next(v for k, v in tr._unpadded_cache.items() if k[1] == n and k[0][0] == (4, 4))
    assert id(const) in got
    assert any(id(v) in got for v in tr._shape_cache.values())
    assert sum(id(v) in got for v in joiner._pos_cache.values()) >= 3          # the three levels of this geometry
    inside = len(holder)
    run(cpu_model, clip, ids)                                                  # outside a scope nothing is appended
    assert len(holder) == inside


def test_keep_alive_scopes_nest_and_hold_once():
    a, b = [], []
    x, y = torch.zeros(3), torch.ones(3)
    with DC.keep_alive(a):
        assert DC.hold(x) is x
        with DC.keep_alive(b):
            DC.hold(y)
            DC.hold(y)
        DC.hold(x)
    DC.hold(y)
    assert [id(v) for v in a] == [id(x), id(y)] and [id(v) for v in b] == [id(y)]


def test_derived_cache_rebuild_keeps_the_image_a_scope_was_handed():
    """DerivedCache.get replaces an entry after a `_version` bump.  The value handed out inside a scope survives the replacement
    while the holder lives, and is freed with it."""
    cache = DC.DerivedCache()
    w = torch.nn.Parameter(torch.arange(6.0).reshape(2, 3))
    holder = []
    with DC.keep_alive(holder):
        v1 = cache.get((w,), lambda: w.detach() * 2)
    r1 = weakref.ref(v1)
    del v1
    with torch.no_grad():
        w.add_(1)
    v2 = cache.get((w,), lambda: w.detach() * 2)
    assert len(cache) == 1 and torch.equal(v2, w.detach() * 2)
    assert r1() is not None and torch.equal(r1(), (w.detach() - 1) * 2)       # the old image, intact
    assert cache.get((w,), lambda: None) is v2 and len(holder) == 1          # a hit outside the scope: nothing appended
    del holder[:]
    gc.collect()
    assert r1() is None


def test_fpn_tap_cache_rebuild_keeps_the_image_a_scope_was_handed(cpu_model):
    dec = cpu_model.spatial_decoder
    conv = dec.lay1
    before = conv.weight.detach().clone()
    holder = []
    try:
        with DC.keep_alive(holder):
            t1 = dec._taps(conv)
        r1, want1 = weakref.ref(t1), t1.clone()
        del t1
        with torch.no_grad():
            conv.weight.mul_(0.5)
        t2 = dec._taps(conv)
        assert torch.equal(t2, want1 * 0.5)
        assert r1() is not None and torch.equal(r1(), want1)
        del holder[:]
        gc.collect()
        assert r1() is None
    finally:
        with torch.no_grad():
            conv.weight.copy_(before)


def test_clip_inferencer_drops_its_graphs_when_the_weights_are_reloaded(synthetic_sd, monkeypatch):
    """ClipInferencer compares one integer per call: a load_state_dict on the model -- or on any part of it -- since the graphs
    were captured drops them all; nothing else does.  (Host side only: the graph dictionaries hold stand-ins here.)"""
    from neurips2023_soc_amd import infer
    model, _, _ = S.build_model(S.default_args(text_encoder_random_init=True, device="cpu"))
    model.load_state_dict(synthetic_sd, strict=False)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    engine = infer.ClipInferencer(model.eval(), "cpu", use_graphs=True)
    epoch = infer.weights_epoch(model)
    assert infer.weights_epoch(model) is epoch                       # installed once
    n_hooks = sum(len(m._load_state_dict_post_hooks) for m in model.modules())
    infer.ClipInferencer(model, "cpu", use_graphs=True)
    assert sum(len(m._load_state_dict_post_hooks) for m in model.modules()) == n_hooks

    def fill():
        engine._graphs[(1, 32, 32, 6)] = object()
        engine._pipes[(1, 32, 32, 6)] = object()
        engine._singles[(1, 32, 32, 6)] = object()

    fill()
    engine._check_weights()
    assert len(engine._graphs) == len(engine._pipes) == len(engine._singles) == 1          # nothing loaded: nothing dropped
    model.load_state_dict(synthetic_sd, strict=False)
    engine._check_weights()
    assert not engine._graphs and not engine._pipes and not engine._singles
    assert engine.stats["weight_reloads_seen"] == 1
    fill()
    engine._check_weights()
    assert len(engine._graphs) == 1
    backbone_sd = {k[len("backbone."):]: v for k, v in synthetic_sd.items() if k.startswith("backbone.")}
    model.backbone.load_state_dict(backbone_sd, strict=False)       # a part of the model (load_kinetics_weights does this)
    engine._check_weights()
    assert not engine._graphs and not engine._pipes and not engine._singles
    fill()
    engine._active = ((1, 32, 32, 6), None, [("tag", None)])        # a clip in flight under the old weights
    model.load_state_dict(synthetic_sd, strict=False)
    with pytest.raises(RuntimeError, match="drain"):
        engine._check_weights()
    engine._active = None
    engine.reset()
    assert not engine._graphs
