"""-m gpu: the forward with valid_indices (the centre-frame protocol of A2D-Sentences / JHMDB-Sentences) against the
reference's golden, the group rule for it, and the JHMDB-Sentences driver end to end."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import neurips2023_soc_amd as S
from neurips2023_soc_amd import center_eval as CE, center_frame as CF, infer_jhmdb as J, postprocessing as P, weights as W
from neurips2023_soc_amd.synthetic_dataset import HashTokenizer

pytestmark = pytest.mark.gpu

FLIP_WINDOW = 6e-5          # tests/test_gpu_forward.py: the reference's own thread-count noise at the decision boundary


def maxdiff(a, b):
    return float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(b).double()).abs().max())


@pytest.fixture(scope="module")
def gpu_model(synthetic_sd):
    assert torch.cuda.is_available()
    model, _, _ = S.build_model(S.default_args(text_encoder_random_init=True))
    model.load_state_dict(synthetic_sd, strict=False)
    return model.cuda().eval()


def run_center(model, cfg, frames, seeds=None):
    """B clips (one per entry of `frames`: the frame of clip b to keep) through model(samples, valid_indices, ...)"""
    seed, T, H, Wd, L = (int(v) for v in cfg)
    seeds = [seed] * len(frames) if seeds is None else seeds
    B = len(frames)
    clips = torch.stack([W.synthetic_clip(s, T, H, Wd) for s in seeds], 1).cuda()            # [T,B,3,H,W]
    samples = S.NestedTensor(clips, torch.zeros(T, B, H, Wd, dtype=torch.bool, device="cuda"), unpadded=True)
    ids = torch.cat([W.synthetic_token_ids(s, L) for s in seeds], 0)
    text = {"input_ids": ids, "attention_mask": torch.ones_like(ids)}
    idx = torch.tensor([f + T * b for b, f in enumerate(frames)], device="cuda")
    return samples, idx, text, [[{"size": torch.tensor([H, Wd])}] * B]


@pytest.mark.parametrize("case", ["centre", "edge"])
def test_forward_with_valid_indices_matches_reference(gpu_model, golden, case):
    """Tolerances: those of test_tiny_config_matches_reference for the same tensors."""
    g = golden("center_forward.npz")
    frame = int(g[f"{case}_frame"])
    assert frame == {"centre": 4, "edge": 0}[case] and int(g["cfg"][1]) == 8
    samples, idx, text, targets = run_center(gpu_model, g["cfg"], [frame])
    out = gpu_model(samples, idx, text, targets)
    torch.cuda.synchronize()
    want = g[f"{case}_pred_masks"]
    assert tuple(out["pred_masks"].shape) == want.shape and want.shape[:3] == (1, 1, 20)       # T = 1 behind the backbone
    d = maxdiff(out["pred_masks"], want)
    print(case, "max|dlogit|", d, "of", np.abs(want).max())
    assert d < 1e-3
    flip = (out["pred_masks"].cpu().numpy() > 0) != (want > 0)
    assert flip.sum() <= 2 and (not flip.any() or np.abs(want[flip]).max() < FLIP_WINDOW)
    assert maxdiff(out["pred_cls"], g[f"{case}_pred_cls"]) < 1e-4
    assert maxdiff(out["pred_boxes"], g[f"{case}_pred_boxes"]) < 1e-5
    assert maxdiff(out["pred_logit"], g[f"{case}_pred_logit"]) < 1e-4
    assert maxdiff(out["text_sentence_feature"], g[f"{case}_text_sentence_feature"]) < 1e-4


def test_the_selected_frame_matters(gpu_model, golden):
    g = golden("center_forward.npz")
    assert maxdiff(g["centre_pred_masks"], g["edge_pred_masks"]) > 1e-2


def test_group_of_two_gives_every_clip_its_single_clip_result(gpu_model, golden):
    """B = 2 with valid_indices = [4, 12] and the VOC module per clip: each clip gets its B = 1 result, within the bound of
    test_group_pipeline_gives_every_clip_its_single_clip_result (1e-4 on the record: masks and class logits)."""
    cfg = golden("center_forward.npz")["cfg"]
    seed = int(cfg[0])
    seeds = [seed, seed + 1]
    samples, idx, text, targets = run_center(gpu_model, cfg, [4, 4], seeds)
    assert idx.tolist() == [4, 12]
    both = gpu_model.forward_tail(gpu_model.forward_head(samples, idx, text), targets, voc_per_clip=True)
    assert tuple(both["pred_masks"].shape[:3]) == (1, 2, 20)
    singles = []
    for b, s in enumerate(seeds):
        one_samples, one_idx, one_text, one_targets = run_center(gpu_model, cfg, [4], [s])
        singles.append(gpu_model(one_samples, one_idx, one_text, one_targets))
    assert maxdiff(singles[0]["pred_masks"], singles[1]["pred_masks"].cpu()) > 1e-2            # the clips really are distinct
    for b in range(2):
        assert maxdiff(both["pred_masks"][:, b:b + 1], singles[b]["pred_masks"].cpu()) < 1e-4
        assert maxdiff(both["pred_cls"][:, b:b + 1], singles[b]["pred_cls"].cpu()) < 1e-4
    # the driver's batched call is this one
    clips = [W.synthetic_clip(s, *(int(v) for v in cfg[1:4])).cuda() for s in seeds]
    out = J.forward_center(gpu_model, clips, [W.synthetic_token_ids(s, int(cfg[4])) for s in seeds])
    assert maxdiff(out["pred_masks"], both["pred_masks"].cpu()) < 1e-4


# --------------------------------------------------------------------------------------------------------------------- driver
def slow_way(model, tokenize, root, samples):
    """Every sample on its own: the eager B = 1 forward, then the post-processor on CPU tensors (the reference's torch ops).
    -> per sample (image id, scores [Q], masks bool [Q,oh,ow], the up-sampled logit behind every mask pixel, ground truth)."""
    post = P.build_postprocessors("jhmdb_sentences")
    frame_dirs, mask_files = J.video_folders(root)
    reader = J.WindowReader("cuda")
    out = []
    for video, frame_path, _, total, query in samples:
        frame = J.frame_number(frame_path)
        clip, orig = reader.window(frame_dirs[video], J.window_frames(frame, total))
        T, _, h, w = clip.shape
        ns = S.NestedTensor(clip[:, None], torch.zeros(T, 1, h, w, dtype=torch.bool, device="cuda"), unpadded=True)
        ids = tokenize(J.clean_query(query))
        o = model(ns, torch.tensor([4], device="cuda"), {"input_ids": ids, "attention_mask": torch.ones_like(ids)},
                  [[{"size": (h, w)}]])
        logits = o["pred_masks"].flatten(0, 1).cpu()
        p = post({"pred_masks": logits, "pred_cls": o["pred_cls"].cpu()}, (h, w), [(h, w)], [orig])[0]
        up = F.interpolate(logits, size=(h, w), mode="bilinear", align_corners=False)
        value = F.interpolate(up[0].unsqueeze(1), size=tuple(orig), mode="nearest")[:, 0]
        gt = J.load_part_masks(mask_files[video])[frame - 1] != 0
        out.append((J.image_id(video, frame), p["scores"].numpy(), p["masks"][:, 0].numpy() > 0, value.numpy(), gt))
    return out


def test_driver_end_to_end(gpu_model, tmp_path, capsys):
    """--make-synthetic 2 --group 2 --save-predictions.  The forward is not bit-repeatable (atomics in library kernels) and a
    group of two gives a clip its single-clip logits to f32 rounding only, so a mask pixel of the driver may differ from the slow
    way's where the slow way's up-sampled logit lies inside FLIP_WINDOW of zero, and nowhere else: with no such pixel in a
    sample's scored mask -- printed below -- its counts, and with none at all the metrics, are EQUAL."""
    root, out_dir = str(tmp_path / "j"), str(tmp_path / "o")
    J.make_synthetic(root, videos=2)
    tokenize = HashTokenizer()
    before = CF.launches
    stats = J.run(gpu_model, tokenize, root, out_dir, device="cuda", group=2, save_predictions=True)
    assert stats["samples"] == 6 and stats["batches"] == 3 and CF.launches == before + 3     # one K6c launch per batch
    printed = capsys.readouterr().out
    with open(os.path.join(out_dir, "metrics.json")) as f:
        metrics = json.load(f)
    assert set(metrics) == {"P@0.5", "P@0.6", "P@0.7", "P@0.8", "P@0.9", "overall_iou", "mean_iou", "num_samples"}
    assert str(stats["metrics"]) in printed and metrics["num_samples"] == 6
    samples = J.read_samples(os.path.join(out_dir, "samples.json"))
    assert samples == J.draw_samples(root, 0)
    with open(os.path.join(out_dir, "ious.csv")) as f:
        rows = [line.split(",") for line in f.read().splitlines()]
    assert rows[0] == ["image_id", "query", "iou", "inter", "pred_area", "gt_area"] and len(rows) == 7
    own_counts = [[int(v) for v in r[3:]] for r in rows[1:]]
    own = CE.metrics(own_counts)                                       # the numbers written are center_eval of the counts written
    assert {k: metrics[k] for k in CE.eval_metrics(own)} == CE.eval_metrics(own)
    assert [float(r[2]) for r in rows[1:]] == own["ious"]

    slow = slow_way(gpu_model, tokenize, root, samples)
    with open(os.path.join(out_dir, "predictions.json")) as f:
        preds = json.load(f)
    assert len(preds) == 6 * 20 and all(p["category_id"] == 1 for p in preds)
    slow_counts, uncertain_total = [], 0
    for n, (iid, scores, masks, value, gt) in enumerate(slow):
        mine = preds[20 * n:20 * n + 20]
        assert all(p["image_id"] == iid == rows[1 + n][0] for p in mine)
        assert np.abs(np.array([p["score"] for p in mine]) - scores).max() < 1e-4
        best = int(CE.select_best(scores[None])[0])
        assert int(rows[1 + n][1]) == best
        for q, p in enumerate(mine):                                   # all 20 queries decode to the slow way's masks
            got = CF.rle_decode(p["segmentation"]["counts"], p["segmentation"]["size"])
            diff = got != masks[q]
            assert diff.sum() <= 2 and (not diff.any() or np.abs(value[q][diff]).max() < FLIP_WINDOW), (iid, q, int(diff.sum()))
        uncertain = int((np.abs(value[best]) < FLIP_WINDOW).sum())
        uncertain_total += uncertain
        want = CE.counts_from_masks(masks[best], gt)
        print(iid, "query", best, "counts", own_counts[n], "slow way", want, "pixels inside the flip window", uncertain)
        assert own_counts[n][2] == want[2]
        assert abs(own_counts[n][0] - want[0]) <= uncertain and abs(own_counts[n][1] - want[1]) <= uncertain
        slow_counts.append(want)
    if uncertain_total == 0 or own_counts == slow_counts:
        assert CE.eval_metrics(CE.metrics(slow_counts)) == {k: metrics[k] for k in CE.eval_metrics(own)}


def test_cli_prints_the_metrics_dict(gpu_model, tmp_path, monkeypatch, capsys):
    """infer --dataset jhmdb --root R --out O --make-synthetic 2 --group 2, in this process and with this module's model in
    place of a freshly built one (building one costs more than the run)."""
    from neurips2023_soc_amd import infer
    seen = {}

    def build(args):
        seen["dataset_name"] = args.dataset_name
        return gpu_model, None, P.build_postprocessors(args.dataset_name)
    monkeypatch.setattr(S, "build_model", build)
    monkeypatch.setattr(W, "load_synthetic", lambda model, seed: None)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    argv = ["--dataset", "jhmdb", "--root", str(tmp_path / "j"), "--out", str(tmp_path / "o"), "--make-synthetic", "2",
            "--group", "2"]
    infer._run_dataset(infer.parse_args(argv))
    lines = capsys.readouterr().out.strip().splitlines()
    assert seen["dataset_name"] == "jhmdb_sentences"
    assert lines[-2].startswith("{'P@0.5':") and "'overall_iou':" in lines[-2] and "'mean_iou':" in lines[-2]
    last = json.loads(lines[-1])
    assert last["samples"] == 6 and last["batches"] == 3 and last["samples_per_s"] > 0
    with open(tmp_path / "o" / "metrics.json") as f:
        assert {k: v for k, v in json.load(f).items() if k != "num_samples"} == last["metrics"]
