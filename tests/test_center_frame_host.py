"""Host side of the centre-frame protocol (JHMDB-Sentences): metrics from counts, uncompressed run lengths, the window and
valid_indices arithmetic, the samples file, the synthetic tree, the post-processor on CPU tensors.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import neurips2023_soc_amd as S
from neurips2023_soc_amd import center_eval as CE, center_frame as CF, infer, infer_jhmdb as J, packed_masks as PM
from neurips2023_soc_amd import postprocessing as P
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def metrics_golden():
    with open(os.path.join(GOLDEN, "center_metrics.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------------ metrics
def test_metrics_equal_the_reference_exactly(metrics_golden):
    g = metrics_golden
    counts = np.array(g["counts"])
    best = CE.select_best(np.array(g["scores"]))
    m = CE.metrics(counts[np.arange(len(best)), best])
    assert m["precision_at_k"] == g["precision_at_k"]
    assert m["overall_iou"] == g["overall_iou"]
    assert m["mean_iou"] == g["mean_iou"]
    assert m["ious"] == g["ious"]
    assert m["num_samples"] == len(g["ious"])
    assert CE.eval_metrics(m) == {**{f"P@{k}": p for k, p in zip((0.5, 0.6, 0.7, 0.8, 0.9), g["precision_at_k"])},
                                  "overall_iou": g["overall_iou"], "mean_iou": g["mean_iou"]}


def test_metrics_edge_cases_of_the_golden(metrics_golden):
    g = metrics_golden
    counts, cases = np.array(g["counts"]), g["cases"]
    best = CE.select_best(np.array(g["scores"]))
    iou = CE.ious(counts[np.arange(len(best)), best])
    n = cases["empty_vs_empty"]
    assert counts[n, best[n]].tolist() == [0, 0, 0] and iou[n] == 1.0
    n = cases["exact_half"]
    inter, area, gt = counts[n, best[n]]
    assert 2 * inter == area + gt - inter and iou[n] > 0.5                   # exactly 1/2 lands above 0.5, as in the reference
    n = cases["just_under_0.6"]
    assert 0.5 < iou[n] < 0.6 and 0.6 - iou[n] < 2e-3
    n = cases["score_tie"]
    scores = g["scores"][n]
    assert scores[0] == scores[1] == max(scores) and best[n] == 1            # the LAST of the tied queries


def test_select_best_and_bad_input():
    assert CE.select_best([[0.1, 0.9, 0.9, 0.2], [0.5, 0.1, 0.2, 0.3], [0.3, 0.3, 0.3, 0.3]]).tolist() == [2, 0, 3]
    with pytest.raises(ValueError):
        CE.select_best(np.zeros((2, 0)))
    with pytest.raises(ValueError):
        CE.metrics(np.zeros((0, 3), np.int64))
    assert CE.counts_from_masks([[1, 1, 0]], [[0, 2, 2]]) == [1, 2, 2]


# ------------------------------------------------------------------------------------------------------------ run lengths
def _rle_reference(mask):
    """transitions of mask.flatten(order='F'); the first run is of zeros"""
    flat = np.asarray(mask, bool).flatten(order="F")
    runs, current, n = [], False, 0
    for v in flat:
        if v != current:
            runs.append(n)
            current, n = v, 0
        n += 1
    runs.append(n)
    return runs


@pytest.mark.parametrize("width", [1, 63, 64, 65])
@pytest.mark.parametrize("kind", ["zeros", "ones", "first_pixel", "random"])
def test_rle_counts_vs_numpy_restatement(width, kind):
    h = 5
    rng = np.random.default_rng(width)
    mask = {"zeros": np.zeros((h, width), bool), "ones": np.ones((h, width), bool),
            "first_pixel": np.arange(h * width).reshape(h, width) == 0, "random": rng.random((h, width)) > 0.5}[kind]
    bits = PM.pack(mask)
    bits[:, -1] |= np.uint8(0x80 if width % 64 else 0)                  # a padding bit that is set must not count
    counts = CF.rle_counts(bits, (h, width))
    assert counts == _rle_reference(mask)
    assert sum(counts) == h * width
    if kind == "zeros":
        assert counts == [h * width]
    if kind == "ones":
        assert counts == [0, h * width]
    if kind == "first_pixel":
        assert counts[0] == 0 and counts[1] == 1
    np.testing.assert_array_equal(CF.rle_decode(counts, (h, width)), mask)
    assert CF.rle_counts(torch.from_numpy(bits), (h, width)) == counts


def test_rle_decode_refuses_a_wrong_size():
    with pytest.raises(ValueError):
        CF.rle_decode([3, 2], (2, 3))


def test_mask_offsets_and_ground_truth_packing():
    original = [(29, 71), (40, 100), (3, 64)]
    offsets, total = CF.mask_offsets(original, 3)
    assert offsets == [0, 3 * 29 * 16, 3 * 29 * 16 + 3 * 40 * 16] and total == offsets[-1] + 3 * 3 * 8
    assert all(o % 8 == 0 for o in offsets)
    rng = np.random.default_rng(0)
    gts = [(rng.random(s) > 0.5).astype(np.uint8) * 3 for s in original]      # any non-zero value is foreground
    flat, off = CF.pack_ground_truth(gts, "cpu")
    for g, o, s in zip(gts, off, original):
        plane = flat[o:o + CF.plane_bytes(s)].view(s[0], PM.row_bytes(s[1]))
        np.testing.assert_array_equal(PM.unpack(plane.numpy(), s[1]), g != 0)


# ------------------------------------------------------------------------------------------------------------ window, samples
def test_window_and_valid_indices_arithmetic():
    assert J.window_frames(1, 30) == [1, 1, 1, 1, 1, 2, 3, 4]                 # first frame: the front is the edge frame repeated
    assert J.window_frames(30, 30) == [26, 27, 28, 29, 30, 30, 30, 30]        # last frame
    assert J.window_frames(15, 30) == [11, 12, 13, 14, 15, 16, 17, 18]        # a middle frame
    assert J.window_frames(2, 3) == [1, 1, 1, 1, 2, 3, 3, 3]
    for frame, total in ((1, 30), (30, 30), (15, 30), (2, 3)):
        w = J.window_frames(frame, total)
        assert len(w) == J.WINDOW and w[J.WINDOW // 2] == frame and all(1 <= i <= total for i in w)
    assert J.valid_indices(1) == [4] and J.valid_indices(3) == [4, 12, 20]
    assert J.clean_query("  A Man   is\tWalking ") == "a man is walking"
    assert J.image_id("video003", 7) == "v_video003_f_7"
    assert J.frame_number("/data/Rename_Images/walk/v/00012.png") == 12


def test_synthetic_tree_round_trip(tmp_path):
    import scipy.io
    root = J.make_synthetic(str(tmp_path / "j"), videos=3, frames=7, height=48, width=64, seed=1)
    rows = J.read_annotations(root)
    assert [v for v, _ in rows] == ["video000", "video001", "video002"]
    with open(os.path.join(root, "jhmdb_annotation.txt")) as f:
        lines = f.read().splitlines()
    assert lines[0] == "video_id,query" and len(lines) == 4
    for (_, q), line in zip(rows, lines[1:]):
        assert line.split(",", 1)[1] == q and J.clean_query(q) != q        # the raw queries need the clean-up
    frame_dirs, mask_files = J.video_folders(root)
    assert sorted(frame_dirs) == sorted(mask_files) == ["video000", "video001", "video002"]
    for v, name in enumerate(sorted(frame_dirs)):
        frames = sorted(os.listdir(frame_dirs[name]))
        assert frames == [f"{i:05d}.png" for i in range(1, 8)]
        masks = J.load_part_masks(mask_files[name])
        raw = scipy.io.loadmat(mask_files[name])["part_mask"]
        assert raw.shape == (48, 64, 7 - v % 2) and masks.shape == (7 - v % 2, 48, 64)
        from neurips2023_soc_amd import synthetic_dataset as SD
        np.testing.assert_array_equal(masks, SD.blob_label_maps(1000 + v, 7 - v % 2, 48, 64, objects=1))
        from neurips2023_soc_amd import clip_io
        assert clip_io.decode_frame(os.path.join(frame_dirs[name], frames[0])).shape == (48, 64, 3)


def test_samples_are_drawn_repeatably_and_round_trip(tmp_path):
    root = J.make_synthetic(str(tmp_path / "j"), videos=2, frames=7, height=32, width=48)
    a, b, c = J.draw_samples(root, seed=3), J.draw_samples(root, seed=3), J.draw_samples(root, seed=4)
    assert a == b and a != c and len(a) == 2 * J.FRAMES_PER_QUERY
    for video, frame_path, masks_path, total, query in a:
        assert total == (7 if video == "video000" else 6)                  # frames beyond the number of masks are ignored
        assert 1 <= J.frame_number(frame_path) <= total and os.path.exists(frame_path) and os.path.exists(masks_path)
    per_video = [J.frame_number(p) for v, p, *_ in a if v == "video001"]
    assert per_video == sorted(per_video) and len(set(per_video)) == 3
    path = str(tmp_path / "samples.json")
    J.write_samples(a, path)
    assert J.read_samples(path) == a


def test_a_reference_format_samples_file_is_accepted(tmp_path):
    """The reference's metadata rows carry ITS paths; only the frame number of frame_path is used."""
    rows = [["video000", "/mnt/other/jhmdb_sentences/Rename_Images/walk/video000/00003.png",
             "/mnt/other/jhmdb_sentences/puppet_mask/walk/video000/puppet_mask.mat", 6, "A man Walks"]]
    path = str(tmp_path / "ref_samples.json")
    with open(path, "w") as f:
        json.dump(rows, f)
    got = J.read_samples(path)
    assert got == [tuple(rows[0])] and J.frame_number(got[0][1]) == 3 and isinstance(got[0][3], int)


# ------------------------------------------------------------------------------------------------------------ post-processor
def test_build_postprocessors_returns_the_centre_frame_class():
    for name in ("a2d_sentences", "jhmdb_sentences"):
        assert isinstance(P.build_postprocessors(name), P.A2DSentencesPostProcess)
    assert isinstance(P.build_postprocessors("ref_youtube_vos"), P.ReferYoutubeVOSPostProcess)
    assert P.build_postprocessors("davis") is None
    with pytest.raises(NotImplementedError):
        P.build_postprocessors("coco")


def test_postprocessor_on_cpu_tensors_equals_the_reference(golden):
    g = golden("center_postprocess.npz")
    post = P.build_postprocessors("jhmdb_sentences")
    for k in range(int(g["n_geometries"])):
        outputs = {"pred_masks": torch.from_numpy(g[f"g{k}_logits"]), "pred_cls": torch.from_numpy(g[f"g{k}_pred_cls"])}
        resized, orig = g[f"g{k}_resized"].tolist(), g[f"g{k}_orig"].tolist()
        out = post(outputs, tuple(g[f"g{k}_padded"].tolist()), resized, orig)
        assert len(out) == len(orig)
        for n, p in enumerate(out):
            want = g[f"g{k}_s{n}_masks"]
            assert p["masks"].dtype == torch.float32 and tuple(p["masks"].shape) == want.shape
            np.testing.assert_array_equal(p["masks"].numpy(), want.astype(np.float32))
            np.testing.assert_array_equal(p["scores"].numpy(), g[f"g{k}_s{n}_scores"])
            assert len(p["rle_masks"]) == want.shape[0]
            for q, rle in enumerate(p["rle_masks"]):
                assert rle["size"] == orig[n]
                np.testing.assert_array_equal(CF.rle_decode(rle["counts"], orig[n]), want[q, 0] != 0)


# ------------------------------------------------------------------------------------------------------------ model, CLI
def test_valid_indices_must_name_one_frame_per_clip():
    model, _, post = S.build_model(S.default_args(text_encoder_random_init=True, device="cpu"))
    model.eval()
    T, B = 8, 1
    samples = S.NestedTensor(torch.zeros(T, B, 3, 32, 32), torch.zeros(T, B, 32, 32, dtype=torch.bool))
    text = {"input_ids": torch.tensor([[0, 5, 2]]), "attention_mask": torch.ones(1, 3, dtype=torch.long)}
    with pytest.raises(ValueError, match=r"\[3, 4\]"):
        model.forward_backbone(samples, torch.tensor([3, 4]), text)            # two frames for one clip
    with pytest.raises(ValueError, match=r"\[8\]"):
        model.forward_backbone(samples, torch.tensor([8]), text)               # a frame of a clip that is not there
    with pytest.raises(ValueError):
        model.forward_backbone(samples, torch.tensor([4.0]), text)
    two = S.NestedTensor(torch.zeros(T, 2, 3, 32, 32), torch.zeros(T, 2, 32, 32, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"\[12, 4\]"):
        model.forward_backbone(two, torch.tensor([12, 4]), text)               # not in clip order
    assert S.SOC._check_valid_indices(torch.tensor([4, 12]), 8, 2).tolist() == [4, 12]


def test_select_valid_frames_selects_every_part_of_the_state():
    n, idx = 16, torch.tensor([4, 12])
    feats = [torch.arange(n * 2 * 3 * 3, dtype=torch.float32).view(n, 3, 3, 2).permute(0, 3, 1, 2) for _ in range(4)]
    state = {"feats": feats, "masks": [torch.zeros(n, 3, 3, dtype=torch.bool) for _ in range(4)],
             "pos": [None] + [torch.randn(n, 4, 3, 3) for _ in range(3)], "sample_mask": torch.zeros(n, 12, 12, dtype=torch.bool),
             "unpadded": True}
    out = S.SOC.select_valid_frames(state, idx)
    for l in range(4):
        assert torch.equal(out["feats"][l], feats[l][idx]) and out["masks"][l].shape[0] == 2
        assert out["feats"][l].permute(0, 2, 3, 1).is_contiguous()             # channels-last maps stay channels-last
    assert out["pos"][0] is None and all(torch.equal(out["pos"][l], state["pos"][l][idx]) for l in (1, 2, 3))
    assert out["sample_mask"].shape[0] == 2 and out["unpadded"] is True
    assert state["feats"][0].shape[0] == n                                     # the state handed in is left as it was


@pytest.mark.parametrize("flags, message", [
    (["--packed-masks"], "--packed-masks applies to --dataset refytb"),
    (["--share-video"], "--share-video applies to --dataset refytb"),
    (["--eval-davis", "GT"], "--eval-davis scores the output of --dataset davis"),
    (["--eval-refytb", "GT"], "--eval-refytb scores the output of --dataset refytb"),
])
def test_flags_of_the_other_drivers_stay_errors(capsys, flags, message):
    with pytest.raises(SystemExit):
        infer.parse_args(["--dataset", "jhmdb", "--root", "r", "--out", "o", *flags])
    assert message in capsys.readouterr().err


def test_jhmdb_arguments_parse_and_a2d_is_not_a_dataset(capsys):
    a = infer.parse_args(["--dataset", "jhmdb", "--root", "r", "--out", "o", "--group", "2", "--samples", "s.json",
                          "--save-predictions", "--seed", "5"])
    assert (a.dataset, a.group, a.samples, a.save_predictions, a.seed) == ("jhmdb", 2, "s.json", True, 5)
    assert infer.parse_args(["--dataset", "jhmdb", "--root", "r", "--out", "o"]).group == 1
    with pytest.raises(SystemExit):
        infer.parse_args(["--dataset", "a2d", "--root", "r", "--out", "o"])
    with pytest.raises(SystemExit):
        infer.parse_args(["--dataset", "refytb", "--root", "r", "--out", "o", "--save-predictions"])
