"""CPU: the host side of the shared-video path -- ClipInferencer(share_video=True) bookkeeping with a stub runner, the static
inputs of graph_runner.shared_group_pipeline_class, and the --share-video flag down to both drivers.  No GPU."""
import json
import os

import pytest
import torch

from neurips2023_soc_amd import graph_runner as G
from neurips2023_soc_amd import infer


class Model:
    num_queries = 1


class StubShared:
    """record row s = (clip id staged, first token of slot s); replay() returns the previous replay's rows (DEPTH 2).  A slot
    that is not staged keeps its previous token, as the real runner's static ids do."""
    made = []

    def __init__(self, model, T, H, W, L, device, slots=4):
        self.CLIPS, self.key = slots, (T, H, W, L)
        self.video, self.tokens = None, [-1.0] * slots
        self.in_head, self.n, self.staged_videos = None, 0, 0
        StubShared.made.append(self)

    def stage_video(self, clip):
        self.video = float(clip.reshape(-1)[0])
        self.staged_videos += 1

    def stage_inputs(self, ids, attn=None, slot=0):
        assert ids.shape[-1] == self.key[3] and (attn is None or attn.shape == ids.shape)
        self.tokens[slot] = float(ids.view(-1)[0])

    def _rows(self):
        return torch.tensor([[self.video, t] for t in self.tokens])

    def replay(self):
        prev, self.in_head = self.in_head, self._rows()
        self.n += 1
        return prev if self.n >= 2 else None

    def flush(self):
        if self.n == 0:
            return []
        rec, self.n, self.in_head = self.in_head, 0, None
        return [rec]


def stub_engine(monkeypatch, group, **kw):
    StubShared.made = []
    monkeypatch.setattr(infer, "shared_group_pipeline_class",
                        lambda slots: (lambda *a: StubShared(*a, slots=slots)))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    eng = infer.ClipInferencer(Model(), "cpu", use_graphs=True, group=group, share_video=True, **kw)
    monkeypatch.setattr(eng, "_unpack", lambda rec, key, tag, osz, packed=None:
                        {"tag": tag, "osz": osz, "video": float(rec[0]), "token": float(rec[1]), "key": key})
    return eng


def call(eng, video, tokens, T=8, H=4, W=6, lengths=None):
    """one submit_expressions: clip filled with `video`, expression e starting with token tokens[e]"""
    clip = torch.full((T, 3, H, W), float(video))
    ids = [torch.full((1, (lengths or [5] * len(tokens))[e]), tok, dtype=torch.long) for e, tok in enumerate(tokens)]
    return eng.submit_expressions(clip, ids, [(video, tok) for tok in tokens], (2 * H, 2 * W))


@pytest.mark.parametrize("group", [1, 2, 4, 8])
def test_slots_split_stale_and_tag_order(monkeypatch, group):
    """Every expression comes back exactly once, under its own tag, in the order given, with its own video and tokens; E > group
    splits into ceil(E / group) replays of ONE staged clip; the rows of stale slots are never handed out."""
    eng = stub_engine(monkeypatch, group)
    calls = [(10, [3, 4, 5]), (11, [6, 7, 8, 9, 10, 11]), (12, [13]), (13, [14, 15, 16, 17])]
    got = []
    for video, tokens in calls:
        got += call(eng, video, tokens)
    got += eng.drain()
    want = [(v, tok) for v, tokens in calls for tok in tokens]
    assert [r["tag"] for r in got] == want
    assert [(int(r["video"]), int(r["token"])) for r in got] == want
    assert all(r["osz"] == (8, 12) for r in got)
    passes = sum(-(-len(tokens) // group) for _, tokens in calls)
    assert eng.stats["shared_video_passes"] == passes and eng.stats["shared_expressions"] == len(want)
    assert eng.stats["stale_slots"] == passes * group - len(want)
    assert eng.stats["group_replays"] == 0 and eng.stats["remainder_singles"] == 0
    assert len(StubShared.made) == 1 and StubShared.made[0].staged_videos == len(calls)      # the clip once per call
    assert eng.drain() == [] and eng._shared_active is None


def test_six_expressions_in_four_slots(monkeypatch):
    eng = stub_engine(monkeypatch, 4)
    first = call(eng, 1, [20, 21, 22, 23, 24, 25])
    assert [r["tag"][1] for r in first] == [20, 21, 22, 23]           # the first replay's, handed out behind the second
    assert [r["tag"][1] for r in eng.drain()] == [24, 25]             # slots 2, 3 of the second replay were stale
    assert eng.stats["shared_video_passes"] == 2 and eng.stats["shared_expressions"] == 6 and eng.stats["stale_slots"] == 2


def test_expressions_are_padded_to_the_longest(monkeypatch):
    eng = stub_engine(monkeypatch, 4)
    ids, attns = eng._pad_expressions([torch.tensor([[0, 7, 2]]), torch.tensor([[0, 8, 9, 9, 2]])], None)
    assert [t.tolist() for t in ids] == [[[0, 7, 2, 1, 1]], [[0, 8, 9, 9, 2]]]
    assert attns[0].tolist() == [[1, 1, 1, 0, 0]] and attns[1] is None
    call(eng, 1, [5, 6], lengths=[3, 7])
    assert StubShared.made[0].key == (8, 4, 6, 7)
    eng.drain()
    eng.pad_tokens_to = 32
    call(eng, 1, [5, 6], lengths=[3, 7])
    assert StubShared.made[1].key == (8, 4, 6, 32)


def test_geometry_change_drains_first(monkeypatch):
    eng = stub_engine(monkeypatch, 4)
    assert call(eng, 1, [2, 3]) == []
    got = call(eng, 2, [4], H=6)                                       # another geometry: video 1's results leave first
    assert [r["tag"] for r in got] == [(1, 2), (1, 3)] and all(r["key"] == (8, 4, 6, 5) for r in got)
    assert [r["tag"] for r in eng.drain()] == [(2, 4)]
    assert len(StubShared.made) == 2


def test_shared_and_plain_streams_do_not_mix(monkeypatch):
    """submit() behind submit_expressions() (and the other way round) drains what is in flight first."""
    eng = stub_engine(monkeypatch, 2)

    class Plain:
        def __init__(self):
            self.slots, self.prev, self.n = [None, None], None, 0

        def stage_inputs(self, clip, ids, attn=None, slot=0):
            self.slots[slot] = float(clip.reshape(-1)[0])

        def replay(self):
            prev, self.prev = self.prev, torch.tensor([[v, 0.0] for v in self.slots])
            self.n += 1
            return prev if self.n >= 2 else None

        def flush(self):
            rec, self.n = self.prev, 0
            return [rec] if rec is not None else []

    plain = Plain()
    monkeypatch.setattr(eng, "_pipeline", lambda key: plain)
    assert call(eng, 1, [2, 3]) == []
    clip = torch.full((8, 3, 4, 6), 50.0)
    got = eng.submit(clip, torch.ones(1, 5, dtype=torch.long), "p0", (8, 12))
    assert [r["tag"] for r in got] == [(1, 2), (1, 3)]
    got = eng.submit(clip + 1, torch.ones(1, 5, dtype=torch.long), "p1", (8, 12))
    assert got == []
    got = call(eng, 7, [8])
    assert [r["tag"] for r in got] == ["p0", "p1"]
    assert [r["tag"] for r in eng.drain()] == [(7, 8)]


def test_shared_pipelines_count_against_max_graphs(monkeypatch):
    eng = stub_engine(monkeypatch, 2, max_graphs=2)
    eng._pipes[(1, 1, 1, 1)] = object()
    for H in (4, 6, 8):
        call(eng, H, [1], H=H)
        assert len(eng._shared) + len(eng._pipes) <= 2
    eng.drain()
    assert list(eng._shared) == [(8, 6, 6, 5), (8, 8, 6, 5)] and not eng._pipes
    # ... and the other way round: a pipeline of submit() pushes the oldest shared one out
    monkeypatch.setattr(infer, "pipeline_class", lambda: (lambda *a: object()))
    monkeypatch.setattr(infer, "group_pipeline_class", lambda n: (lambda *a: object()))
    eng._pipeline((8, 4, 4, 5))
    assert list(eng._shared) == [(8, 8, 6, 5)] and list(eng._pipes) == [(8, 4, 4, 5)]


def test_share_video_off_constructs_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a shared-video pipeline was constructed with share_video=False")
    monkeypatch.setattr(infer, "shared_group_pipeline_class", boom)
    eng = infer.ClipInferencer(Model(), "cpu", use_graphs=True, group=2)
    assert eng.share_video is False and eng._shared == {} and eng._shared_active is None
    with pytest.raises(RuntimeError, match="share_video"):
        eng.submit_expressions(torch.zeros(2, 3, 4, 4), [torch.ones(1, 3, dtype=torch.long)], ["t"])
    with pytest.raises(RuntimeError, match="share_video"):
        eng.run_expressions(torch.zeros(2, 3, 4, 4), [torch.ones(1, 3, dtype=torch.long)])
    assert eng.drain() == [] and eng.stats["shared_video_passes"] == 0
    eager = infer.ClipInferencer(Model(), "cpu", use_graphs=False, share_video=True)
    with pytest.raises(RuntimeError, match="use_graphs"):
        eager.submit_expressions(torch.zeros(2, 3, 4, 4), [torch.ones(1, 3, dtype=torch.long)], ["t"])


@pytest.mark.parametrize("slots", [1, 3])
def test_shared_runner_static_inputs_and_staging(slots):
    """ONE clip, `slots` token rows and records; stage_video / stage_inputs fill them; the attention mask of a slot goes back to
    ones when ids are staged without one."""
    cls = G.shared_group_pipeline_class(slots)
    assert issubclass(cls, G.PairPipelinedClipGraph) and cls.CLIPS == slots and cls.DEPTH == 2
    assert cls.replay is G.PipelinedClipGraph.replay and cls.flush is G.PipelinedClipGraph.flush
    assert cls._tail_body is G.PairPipelinedClipGraph._tail_body and cls._build is G.PipelinedClipGraph._build
    T, H, W, L = 2, 8, 8, 5
    g = object.__new__(cls)
    g._allocate(Model(), T, H, W, L, "cpu")
    assert g.clip.shape == (T, 1, 3, H, W) and g.pad.shape == (T, 1, H, W) and g.pad.dtype == torch.bool and not g.pad.any()
    assert g.ids.shape == g.attn.shape == (slots, L) and g.record.dim() == 2 and g.record.shape[0] == slots
    assert len(g.targets) == T and len(g.targets[0]) == 1
    clip = torch.randn(T, 3, H, W)
    g.stage_video(clip)
    assert torch.equal(g.clip[:, 0], clip)
    g.stage_video(2 * clip[:, None])
    assert torch.equal(g.clip[:, 0], 2 * clip)
    ids, mask = torch.arange(2, 2 + L), torch.tensor([1, 1, 1, 0, 0])
    s = slots - 1
    g.stage_inputs(ids[None], mask[None], slot=s)
    assert torch.equal(g.ids[s], ids) and torch.equal(g.attn[s], mask)
    g.stage_inputs(ids + 1, slot=s)
    assert torch.equal(g.ids[s], ids + 1) and bool((g.attn == 1).all())
    if slots > 1:
        assert bool((g.ids[0] == 1).all())                            # never staged
    with pytest.raises(ValueError):
        G.shared_group_pipeline_class(0)


def test_share_video_flag_parses():
    a = infer.parse_args(["--dataset", "refytb", "--root", "r", "--out", "o", "--share-video"])
    assert a.share_video is True
    assert infer.parse_args(["--dataset", "davis", "--root", "r", "--out", "o"]).share_video is False
    with pytest.raises(SystemExit):
        infer.parse_args(["--share-video"])                            # the clip stream has no expressions to share


@pytest.mark.parametrize("dataset", ["refytb", "davis"])
@pytest.mark.parametrize("flag", [True, False])
def test_share_video_flag_reaches_the_driver(monkeypatch, tmp_path, dataset, flag):
    import neurips2023_soc_amd as S
    from neurips2023_soc_amd import infer_davis, infer_refytb, weights
    meta = tmp_path / "meta_expressions" / "valid"
    meta.mkdir(parents=True)
    (meta / "meta_expressions.json").write_text(json.dumps({"videos": {}}))
    seen = {}

    class FakeModel:
        def to(self, dev):
            return self

        def eval(self):
            return self

    class FakeEngine:
        def __init__(self, model, dev, **kw):
            seen["engine"] = kw

    def fake_run(model, tokenize, root, out, rank, world, dev, engine=None, **kw):
        seen["run"] = kw
        return {"expressions": 1, "seconds": 1.0}

    monkeypatch.setattr(S, "build_model", lambda args: (FakeModel(), None, None))
    monkeypatch.setattr(weights, "load_synthetic", lambda model, seed: None)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(infer, "ClipInferencer", FakeEngine)
    monkeypatch.setattr(infer_refytb if dataset == "refytb" else infer_davis, "run", fake_run)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    argv = ["--dataset", dataset, "--root", str(tmp_path), "--out", os.path.join(str(tmp_path), "out"), "--graphs", "--group", "4"]
    infer._run_dataset(infer.parse_args(argv + (["--share-video"] if flag else [])))
    assert seen["engine"]["share_video"] is flag and seen["engine"]["group"] == 4
    assert seen["run"].get("share_video", False) is flag
