"""-m gpu: the shared-video forward -- ONE pass over the video side of the model for all expressions of a clip
(SOC.forward_expressions, graph_runner.shared_group_pipeline_class, ClipInferencer(share_video=True)).  Every expression gets
what the one-expression forward of (clip, expression) gives, within the bound the project applies to a launch group's records
against one-clip records (1e-4), with the same selected query; expression 0 is the goldens' and meets them."""
import numpy as np
import pytest
import torch

import neurips2023_soc_amd as S
from neurips2023_soc_amd import clip_parallel as CP, postprocessing as P, weights as W
from tests.golden_utils import sub

pytestmark = pytest.mark.gpu

TOL = 1e-4                 # a group's records against one-clip records (test_group_pipeline_gives_every_clip_its_single_clip_result)
FLIP_WINDOW = 6e-5         # tests/test_gpu_forward.py
KEYS = ("pred_masks", "pred_cls", "pred_boxes", "pred_logit", "text_sentence_feature")
BATCH_DIM = {"pred_masks": 1, "pred_cls": 1, "pred_boxes": 1, "pred_logit": 0, "text_sentence_feature": 0}
PAD_ID = 1


def maxdiff(a, b):
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max())


@pytest.fixture(scope="module")
def gpu_model(synthetic_sd):
    assert torch.cuda.is_available()
    model, _, _ = S.build_model(S.default_args(text_encoder_random_init=True))
    model.load_state_dict(synthetic_sd, strict=False)
    return model.cuda().eval()


def expressions(seed, L, E):
    """E distinct expressions of different lengths: expression 0 is the golden's (seed, L); -> [ids [1,L_e]]"""
    lengths = [L, L + 2, max(3, L - 3), L + 1, L + 3, max(3, L - 1), L + 4, L]
    return [W.synthetic_token_ids(seed + e, lengths[e % len(lengths)]).cuda() for e in range(E)]


def padded(ids):
    """-> (input_ids [E,Lmax], attention_mask [E,Lmax]): <pad> and mask 0 behind the shorter expressions"""
    L = max(t.shape[-1] for t in ids)
    rows = torch.full((len(ids), L), PAD_ID, dtype=torch.long, device=ids[0].device)
    attn = torch.zeros_like(rows)
    for e, t_ in enumerate(ids):
        rows[e, :t_.shape[-1]] = t_[0]
        attn[e, :t_.shape[-1]] = 1
    return rows, attn


def samples_of(clip):
    T, _, H, Wd = clip.shape
    return S.NestedTensor(clip[:, None].contiguous(), torch.zeros(T, 1, H, Wd, dtype=torch.bool, device=clip.device), unpadded=True)


def one_expression(model, clip, ids):
    T, _, H, Wd = clip.shape
    out = model(samples_of(clip), None, {"input_ids": ids, "attention_mask": torch.ones_like(ids)},
                [[{"size": (H, Wd)}] for _ in range(T)])
    return {k: out[k].clone() for k in KEYS}


def check_eager(model, cfg, E):
    seed, T, H, Wd, L = (int(v) for v in cfg)
    clip = W.synthetic_clip(seed, T, H, Wd).cuda()
    ids = expressions(seed, L, E)
    want = [one_expression(model, clip, t_) for t_ in ids]
    rows, attn = padded(ids)
    out = model.forward_expressions(samples_of(clip), {"input_ids": rows, "attention_mask": attn},
                                    [[{"size": (H, Wd)}] for _ in range(T)])
    torch.cuda.synchronize()
    assert out["pred_masks"].shape[:3] == (T, E, 20) and out["pred_logit"].shape[0] == E
    for e in range(E):
        got = {k: out[k].narrow(BATCH_DIM[k], e, 1) for k in KEYS}
        for k in KEYS:
            d = maxdiff(got[k], want[e][k])
            print(f"E={E} T={T} expression {e} {k}: max diff {d:.3e}")
            assert d < TOL, (e, k, d)
        assert int(P.select_trajectory(got)[0]) == int(P.select_trajectory(want[e])[0]), e
    for e in range(1, E):                                  # the expressions really differ
        assert maxdiff(want[e]["pred_masks"], want[0]["pred_masks"]) > 1e-2, e
    return {k: out[k].narrow(BATCH_DIM[k], 0, 1) for k in KEYS}


@pytest.mark.parametrize("E", [2, 4])
def test_forward_expressions_tiny(gpu_model, golden, E):
    """E != T = 3 on purpose: a '(b t)' / '(t b)' mix-up of the expression and frame axes cannot pass."""
    g = golden("tiny_forward.npz")
    first = check_eager(gpu_model, g["cfg"], E)
    d = maxdiff(first["pred_masks"], g["pred_masks"])               # expression 0: as test_tiny_config_matches_reference
    assert d < 1e-3
    flip = (first["pred_masks"].cpu().numpy() > 0) != (g["pred_masks"] > 0)
    assert flip.sum() <= 2 and (not flip.any() or np.abs(g["pred_masks"][flip]).max() < FLIP_WINDOW)
    assert maxdiff(first["pred_cls"], g["pred_cls"]) < 1e-4
    assert maxdiff(first["pred_boxes"], g["pred_boxes"]) < 1e-5
    assert maxdiff(first["pred_logit"], g["pred_logit"]) < 1e-4
    assert maxdiff(first["text_sentence_feature"], g["text_sentence_feature"]) < 1e-4


def test_forward_expressions_t10(gpu_model, golden):
    """T = 10: the temporal shift of Video-Swin and the padded last window."""
    g = golden("t10_forward.npz")
    first = check_eager(gpu_model, g["cfg"], 2)
    assert maxdiff(sub(first["pred_masks"], 1 << 16), g["pred_masks_sub"]) < 1e-3
    assert maxdiff(first["pred_cls"], g["pred_cls"]) < 1e-4
    assert maxdiff(first["pred_boxes"], g["pred_boxes"]) < 1e-5
    assert maxdiff(first["pred_logit"], g["pred_logit"]) < 1e-4


def test_forward_video_shared_takes_one_clip(gpu_model):
    clip = W.synthetic_clip(3, 3, 64, 96).cuda()
    two = S.NestedTensor(torch.stack([clip, clip], 1), torch.zeros(3, 2, 64, 96, dtype=torch.bool, device="cuda"), unpadded=True)
    with pytest.raises(ValueError, match="one clip"):
        gpu_model.forward_video_shared(two)


@pytest.fixture(scope="module")
def tiny_stream(gpu_model, golden):
    """Two videos of the tiny geometry, four expressions each (padded to one length), and the one-clip ClipGraph's record of
    every (video, expression) -- computed once, shared by the pipeline and the engine tests."""
    from neurips2023_soc_amd.graph_runner import ClipGraph
    seed, T, H, Wd, L = (int(v) for v in golden("tiny_forward.npz")["cfg"])
    clips = {"A": W.synthetic_clip(seed, T, H, Wd).cuda(), "B": W.synthetic_clip(seed + 50, T, H, Wd).cuda()}
    raw = expressions(seed, L, 6)
    rows, attn = padded(raw)
    Lp = rows.shape[1]
    plain = ClipGraph(gpu_model, T, H, Wd, Lp, "cuda")
    want = {}
    for v, clip in clips.items():
        for e in range(len(raw)):
            plain.run(clip, rows[e:e + 1], attn[e:e + 1])
            want[v, e] = plain.record.clone()
    torch.cuda.synchronize()
    del plain
    assert maxdiff(want["A", 0], want["B", 0]) > 1e-2 and maxdiff(want["A", 0], want["A", 1]) > 1e-2
    return {"geom": (T, H, Wd, Lp), "clips": clips, "raw": raw, "rows": rows, "attn": attn, "want": want}


def test_shared_pipeline_four_slots(gpu_model, tiny_stream):
    """Video A with 3 expressions (one stale slot), video B with 4, A again with 1: every record within 1e-4 of ClipGraph's
    one-clip record with the same query; results arrive one replay late, flush returns the last; a stale slot's row is what
    its stale tokens give for the NEW video (so a caller that handed it out would hand out a wrong answer) and is never
    among the rows a caller takes."""
    from neurips2023_soc_amd.graph_runner import PairPipelinedClipGraph, shared_group_pipeline_class
    s = tiny_stream
    T, H, Wd, Lp = s["geom"]
    pipe = shared_group_pipeline_class(4)(gpu_model, T, H, Wd, Lp, "cuda")
    assert isinstance(pipe, PairPipelinedClipGraph) and pipe.CLIPS == 4 and pipe.flush() == []
    assert pipe.clip.shape == (T, 1, 3, H, Wd) and pipe.ids.shape == (4, Lp) and pipe.record.shape[0] == 4
    plan = [("A", [0, 1, 2]), ("B", [3, 2, 1, 0]), ("A", [4])]
    got = []
    for i, (v, es) in enumerate(plan):
        pipe.stage_video(s["clips"][v])
        for slot, e in enumerate(es):
            pipe.stage_inputs(s["rows"][e:e + 1], s["attn"][e:e + 1], slot=slot)
        rec = pipe.replay()
        assert (rec is None) == (i == 0)                 # one replay late
        if rec is not None:
            got.append(rec.clone())
    rest = pipe.flush()
    assert len(rest) == 1 and pipe.flush() == []
    got.append(rest[0])
    for (v, es), rec in zip(plan, got):
        assert rec.shape[0] == 4
        for slot, e in enumerate(es):
            want = s["want"][v, e]
            assert int(rec[slot, 0]) == int(want[0]), (v, e)
            d = maxdiff(rec[slot], want)
            print(f"video {v} expression {e} slot {slot}: max diff {d:.3e}")
            assert d < TOL, (v, e, d)
    # the stale slots of the last replay (video A) still hold B's tokens 2, 1, 0 in slots 1..3
    for slot, e in ((1, 2), (2, 1), (3, 0)):
        assert maxdiff(got[2][slot], s["want"]["A", e]) < TOL


def test_engine_share_video(gpu_model, tiny_stream):
    """E = 6 through group = 4: two passes (4 + 2), tags in order, packed masks equal pack() of the byte masks of the same
    run, and the eager run_expressions gives the same queries and logits."""
    from neurips2023_soc_amd import packed_masks as PM
    from neurips2023_soc_amd.infer import ClipInferencer
    s = tiny_stream
    T, H, Wd, Lp = s["geom"]
    clip, raw = s["clips"]["A"], s["raw"]
    osz = (2 * H + 1, 2 * Wd + 3)
    tags = [f"e{e}" for e in range(6)]

    def stream(packed):
        eng = ClipInferencer(gpu_model, "cuda", use_graphs=True, group=4, pad_tokens_to=Lp, share_video=True, packed_masks=packed)

        def keep(results):           # 'mask_logits' is a view of the graph's record: copy before the next replay
            return [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()} for r in results]
        res = keep(eng.submit_expressions(clip, raw, tags, osz))
        assert len(res) == 4         # the first replay's expressions, handed out behind the second
        res += keep(eng.drain())
        assert eng.stats["shared_video_passes"] == 2 and eng.stats["shared_expressions"] == 6 and eng.stats["stale_slots"] == 2
        assert eng.drain() == []
        return res

    plain = stream(False)
    assert [r["tag"] for r in plain] == tags
    hm, wm = -(-H // 4), -(-Wd // 4)
    for e, r in enumerate(plain):
        q, cls, masks = CP.unpack_record(s["want"]["A", e].cpu(), T, 20, hm, wm)
        assert int(r["query"]) == q
        assert maxdiff(r["mask_logits"], masks) < TOL and maxdiff(r["pred_cls"], cls) < TOL
        assert r["masks"].shape == (T, *osz) and r["masks"].dtype == torch.bool
    packed = stream(True)
    assert [r["tag"] for r in packed] == tags
    for r, p in zip(plain, packed):
        assert "masks" not in p and p["mask_size"] == osz and int(p["query"]) == int(r["query"])
        assert torch.equal(p["masks_packed"], PM.pack(P.upsample_and_threshold(p["mask_logits"], osz)))   # the same run's logits
    eager = ClipInferencer(gpu_model, "cuda", use_graphs=False, share_video=True)
    res = eager.run_expressions(clip, raw, osz)
    assert len(res) == 6 and eager.stats["shared_video_passes"] == 1 and eager.stats["shared_expressions"] == 6
    for r, want in zip(res, plain):
        assert int(r["query"]) == int(want["query"])
        assert maxdiff(r["mask_logits"], want["mask_logits"]) < TOL
