"""Per-expression J&F (refytb_eval, eval_refytb, the --eval-refytb flag) without a GPU: the host tables from the golden's
counts, the readers and their errors, the command lines, the synthetic ground truth.  Every comparison is exact.
Nothing here reads the reference checkout or oracle/."""
import json
import os

import numpy as np
import pytest
import torch

from neurips2023_soc_amd import davis_eval as DE
from neurips2023_soc_amd import packed_masks as PM
from neurips2023_soc_amd import refytb_eval as RE
from neurips2023_soc_amd import synthetic_dataset as SD
from tests.test_gpu_davis_eval import oracle_counts

GOLDEN = "refytb_jf_cases.npz"


def oracle_counts_bits(gt, obj_ids, exp_obj, pred, r, use_void=True):
    """The numpy oracle of the DAVIS tests on a one-object label map per expression: gt uint8 [T,H,W], pred bool [E,T,H,W] ->
    int32 [E,T,6].  The ground truth keeps its 255s, the named object becomes label 1, everything else background."""
    out = []
    for e, k in enumerate(exp_obj):
        one = np.where(gt == 255, 255, gt == obj_ids[k]).astype(np.uint8)
        out.append(oracle_counts(one, pred[e].astype(np.uint8), 1, 1, r, use_void=use_void, pairs=False)[0])
    return np.stack(out)


def case_of(g, c):
    gt = g[f"{c}_gt"]
    r, use_void = (int(v) for v in g[f"{c}_cfg"])
    return gt, g[f"{c}_obj_ids"].tolist(), g[f"{c}_exp_obj"].tolist(), g[f"{c}_pred_bits"], r, bool(use_void)


def write_tree(g, root, results, annotations_level=False):
    """The golden's small tree as files: ground truth under `root`, the driver's result layout under `results`."""
    from PIL import Image
    meta = {"videos": {}}
    for v in (str(v) for v in g["tree_videos"]):
        gt, frames = g[f"tree_gt_{v}"], [str(f) for f in g[f"tree_frames_{v}"]]
        exps = [(str(e), int(o)) for e, o in zip(g[f"tree_exps_{v}"], g[f"tree_objs_{v}"])]
        pred = PM.unpack(g[f"tree_pred_bits_{v}"], gt.shape[2])
        os.makedirs(os.path.join(root, "valid", "Annotations", v))
        for t, frame in enumerate(frames):
            Image.fromarray(gt[t]).save(os.path.join(root, "valid", "Annotations", v, frame + ".png"))
        for e, (exp_id, _) in enumerate(exps):
            d = os.path.join(results, "Annotations" if annotations_level else "", v, exp_id)
            os.makedirs(d)
            for t, frame in enumerate(frames):
                Image.fromarray(pred[e, t].astype(np.uint8) * 255, mode="L").save(os.path.join(d, frame + ".png"))
        meta["videos"][v] = {"frames": frames, "expressions": {e: {"exp": f"object {o}", "obj_id": o} for e, o in exps}}
    os.makedirs(os.path.join(root, "meta_expressions", "valid"))
    with open(os.path.join(root, "meta_expressions", "valid", "meta_expressions.json"), "w") as f:
        json.dump(meta, f)
    return meta


def result_from_golden_counts(g, order=None):
    res = RE.RefYtbJF()
    for v in (order or [str(v) for v in g["tree_videos"]]):
        res.add_counts(v, [str(e) for e in g[f"tree_exps_{v}"]], g[f"tree_objs_{v}"].tolist(), g[f"tree_counts_{v}"])
    return res


def test_jf_and_statistics_from_the_golden_counts(golden):
    g = golden(GOLDEN)
    for c in (str(c) for c in g["cases"]):
        j, f = DE.jf_from_counts(g[f"{c}_counts"])
        assert np.array_equal(j, g[f"{c}_J"]) and np.array_equal(f, g[f"{c}_F"]), c
        for e in range(len(j)):
            assert list(DE.db_statistics(j[e])) == g[f"{c}_stats"][e, 0].tolist(), (c, e)
            assert list(DE.db_statistics(f[e])) == g[f"{c}_stats"][e, 1].tolist(), (c, e)


def test_tables_from_the_golden_counts_equal_the_golden_row_and_csv_texts(golden, tmp_path):
    g = golden(GOLDEN)
    videos = [str(v) for v in g["tree_videos"]]
    assert videos != sorted(videos)                       # the golden lists them unsorted: the tables sort
    for order in (videos, sorted(videos)):
        res = result_from_golden_counts(g, order)
        assert res.global_row() == g["tree_global"].tolist()
        rows = res.per_expression()
        assert [[r[0], r[1], str(r[2]), repr(r[3]), repr(r[4])] for r in rows] == g["tree_rows"].tolist()
        assert RE.csv_texts(res) == (str(g["tree_csv_global"]), str(g["tree_csv_exp"]))
    assert [r[0] for r in rows] == sorted(r[0] for r in rows)
    assert [r[1] for r in rows if r[0] == "zebra"] == ["2", "0", "1"]          # the JSON's order, not sorted
    paths = RE.write_csvs(res, str(tmp_path), "valid")
    assert [os.path.basename(p) for p in paths] == ["global_results-valid.csv", "per-expression_results-valid.csv"]
    assert open(paths[0]).read() == str(g["tree_csv_global"]) and open(paths[1]).read() == str(g["tree_csv_exp"])
    assert str(g["tree_csv_exp"]).splitlines()[0] == "Video,Expression,Object,J-Mean,F-Mean"
    assert "J&F-Mean" in RE.format_tables(res, "valid")
    with pytest.raises(ValueError, match="do not match 2 expressions"):
        RE.RefYtbJF().add_counts("zebra", ["0", "1"], [1, 2], g["tree_counts_zebra"])


def test_the_oracle_gives_the_golden_counts_on_the_small_cases(golden):
    """Pins the one-object-label-map form of the oracle (the GPU file's second yardstick) to the reference-made golden."""
    g = golden(GOLDEN)
    for c in ("s97x130", "h5_lt_r", "w1", "degenerate", "e5_void", "e5_novoid"):
        gt, obj_ids, exp_obj, bits, r, use_void = case_of(g, c)
        want = oracle_counts_bits(gt, obj_ids, exp_obj, PM.unpack(bits, gt.shape[2]), r, use_void)
        assert np.array_equal(want, g[f"{c}_counts"]), c
    assert g["e5_void_exp_obj"].tolist() == [2, 0, 2, 1, 3] and not (g["e5_void_gt"] == g["e5_void_obj_ids"][3]).any()


def test_object_index():
    assert RE.object_index([7, 3, 7, 254, 3]) == ([3, 7, 254], [1, 0, 1, 2, 0])
    for bad in (0, 255, -1, 300):
        with pytest.raises(ValueError, match="not an object label"):
            RE.object_index([1, bad])


def test_reader_reads_the_tree_and_packs_as_pack_does(golden, tmp_path):
    g = golden(GOLDEN)
    root, results = str(tmp_path / "gt"), str(tmp_path / "runs")
    write_tree(g, root, results)
    ds = RE.RefYtbDataset(root, "valid")
    assert ds.videos == sorted(str(v) for v in g["tree_videos"])
    assert ds.expressions("zebra") == [("2", 1), ("0", 2), ("1", 1)]
    for v in ds.videos:
        gt = ds.masks(v)
        assert gt.dtype == np.uint8 and np.array_equal(gt, g[f"tree_gt_{v}"])
        for e, (exp_id, _) in enumerate(ds.expressions(v)):
            bits = RE.read_results_packed(results, v, exp_id, ds.frames(v), gt.shape[1:])
            want = PM.unpack(g[f"tree_pred_bits_{v}"], gt.shape[2])[e]
            assert bits.dtype == np.uint8 and np.array_equal(bits, PM.pack(want)) and np.array_equal(bits, g[f"tree_pred_bits_{v}"][e])
    assert RE.RefYtbDataset(root, "valid", videos=["zebra"]).videos == ["zebra"]
    # the reference's own layout has an Annotations level in front of the videos
    other = str(tmp_path / "runs_ref")
    write_tree(g, str(tmp_path / "gt2"), other, annotations_level=True)
    assert np.array_equal(RE.read_results_packed(other, "bike", "0", ds.frames("bike"), g["tree_gt_bike"].shape[1:]),
                          g["tree_pred_bits_bike"][0])


def test_reader_errors_name_the_file_or_key(golden, tmp_path):
    from PIL import Image
    g = golden(GOLDEN)
    root, results = str(tmp_path / "gt"), str(tmp_path / "runs")
    meta = write_tree(g, root, results)
    ds = RE.RefYtbDataset(root, "valid")
    shape = g["tree_gt_bike"].shape[1:]
    # a missing result frame, a result of another size
    gone = os.path.join(results, "bike", "1", "00002.png")
    os.remove(gone)
    with pytest.raises(FileNotFoundError, match="bike/1/00002.png"):
        RE.read_results_packed(results, "bike", "1", ds.frames("bike"), shape)
    Image.fromarray(np.zeros((shape[0], shape[1] + 1), dtype=np.uint8)).save(gone)
    with pytest.raises(ValueError, match=r"bike/1/00002.png: size \(50, 71\) does not match the ground truth \(50, 70\)"):
        RE.read_results_packed(results, "bike", "1", ds.frames("bike"), shape)
    # a missing ground-truth frame, a ground-truth frame of another size
    target = os.path.join(root, "valid", "Annotations", "zebra", "00010.png")
    os.remove(target)
    with pytest.raises(FileNotFoundError, match="Annotations/zebra/00010.png"):
        ds.masks("zebra")
    Image.fromarray(np.zeros((61, 100), dtype=np.uint8)).save(target)
    with pytest.raises(ValueError, match="Annotations/zebra/00010.png: size"):
        ds.masks("zebra")
    # an expression without obj_id, a video the JSON does not have, no annotations, no JSON
    del meta["videos"]["zebra"]["expressions"]["0"]["obj_id"]
    with open(ds.meta_path, "w") as f:
        json.dump(meta, f)
    with pytest.raises(KeyError, match=r"videos\['zebra'\]\['expressions'\]\['0'\] has no 'obj_id'"):
        RE.RefYtbDataset(root, "valid").expressions("zebra")
    with pytest.raises(KeyError, match="no video 'camel'"):
        RE.RefYtbDataset(root, "valid", videos=["camel"])
    with pytest.raises(FileNotFoundError, match="test/Annotations|meta_expressions/test"):
        RE.RefYtbDataset(root, "test")
    os.makedirs(os.path.join(root, "meta_expressions", "train"))
    with open(os.path.join(root, "meta_expressions", "train", "meta_expressions.json"), "w") as f:
        json.dump(meta, f)
    with pytest.raises(FileNotFoundError, match="train/Annotations not found"):
        RE.RefYtbDataset(root, "train")


def test_synthetic_annotations_round_trip_through_the_reader(tmp_path):
    root = SD.make_dataset(str(tmp_path / "data"), videos=2, frames=3, height=48, width=80, expressions=[3, 1], seed=4)
    meta_path = os.path.join(root, "meta_expressions", "valid", "meta_expressions.json")
    before = open(meta_path).read()
    # into another directory: the data tree stays as it is
    other = SD.make_refytb_annotations(root, "valid", objects=2, seed=4, void=True, out_root=str(tmp_path / "gt"))
    assert other == str(tmp_path / "gt") and open(meta_path).read() == before
    ds = RE.RefYtbDataset(other, "valid")
    assert ds.videos == ["video000", "video001"]
    assert ds.expressions("video000") == [("0", 1), ("1", 2), ("2", 1)] and ds.expressions("video001") == [("0", 1)]
    for v, name in enumerate(ds.videos):
        maps = ds.masks(name)
        assert np.array_equal(maps, SD.blob_label_maps(4 * 1000 + v, 3, 48, 80, 2, void=True))
        assert ds.frames(name) == json.loads(before)["videos"][name]["frames"]
    assert (ds.masks("video000") == 255).any()
    # in place: the tree's own JSON gains the obj_ids, expressions and frames unchanged
    assert SD.make_refytb_annotations(root, "valid", objects=2, seed=4) == root
    after = json.load(open(meta_path))
    for name, item in json.loads(before)["videos"].items():
        assert after["videos"][name]["frames"] == item["frames"]
        assert {k: v["exp"] for k, v in after["videos"][name]["expressions"].items()} == \
               {k: v["exp"] for k, v in item["expressions"].items()}
    assert RE.RefYtbDataset(root, "valid").expressions("video000") == [("0", 1), ("1", 2), ("2", 1)]
    assert not (RE.RefYtbDataset(root, "valid").masks("video000") == 255).any()


def test_eval_refytb_command_line_argument_errors(capsys):
    from neurips2023_soc_amd import eval_refytb
    for argv in ([], ["--results_path", "x"], ["--root", "y"], ["--results_path", "x", "--root", "y", "--bound-th", "0"],
                 ["--results_path", "x", "--root", "y", "--bound-th", "2.5"], ["--results_path", "x", "--root", "y", "--void"]):
        with pytest.raises(SystemExit) as exc:
            eval_refytb.parse_args(argv)
        assert exc.value.code == 2, argv
    capsys.readouterr()
    a = eval_refytb.parse_args(["--results_path", "x", "--root", "y"])
    assert (a.split, a.no_void, a.bound_th) == ("valid", False, 0.008)
    a = eval_refytb.parse_args(["--results_path", "x", "--root", "y", "--split", "train", "--no-void", "--bound-th", "3"])
    assert (a.split, a.no_void, a.bound_th) == ("train", True, 3.0)
    with pytest.raises(FileNotFoundError, match="meta_expressions.json not found"):
        eval_refytb.main(["--results_path", "x", "--root", "/nonexistent-root"])


def test_infer_flag_belongs_to_the_refytb_driver(capsys):
    from neurips2023_soc_amd import infer
    for argv in (["--dataset", "davis", "--eval-refytb", "GT"], ["--eval-refytb", "GT"]):
        with pytest.raises(SystemExit) as exc:
            infer.parse_args(argv)
        assert exc.value.code == 2
        assert "--eval-refytb scores the output of --dataset refytb" in capsys.readouterr().err
    a = infer.parse_args(["--dataset", "refytb", "--eval-refytb", "GT", "--packed-masks"])
    assert a.eval_refytb == "GT" and a.packed_masks
    assert infer.parse_args(["--dataset", "refytb"]).eval_refytb is None


def test_driver_hook_refuses_more_than_one_process_and_a_tree_without_obj_id(tmp_path):
    from neurips2023_soc_amd import infer_refytb
    root = SD.make_dataset(str(tmp_path / "data"), videos=1, frames=2, height=48, width=80, expressions=2)
    with pytest.raises(ValueError, match="world = 1"):
        infer_refytb.run(None, None, root, str(tmp_path / "out"), world=2, eval_root=root)
    os.makedirs(os.path.join(root, "valid", "Annotations"))
    with pytest.raises(KeyError, match="has no 'obj_id'"):
        infer_refytb._Scorer(root, "valid", ["video000"], "cpu")


def test_scorer_reads_evenly_spaced_slices_in_place_and_copies_anything_else():
    from neurips2023_soc_amd.infer_refytb import _Scorer
    group = torch.zeros(4, 2, 5, 16, dtype=torch.uint8)              # a launch group's [B,T,H0,RB]
    first, stride = _Scorer.in_place([group[1], group[2], group[3]])
    assert first.data_ptr() == group[1].data_ptr() and stride == 2 * 5 * 16
    first, stride = _Scorer.in_place([group[0], group[2]])             # every other slot: still evenly spaced
    assert first.data_ptr() == group[0].data_ptr() and stride == 2 * 2 * 5 * 16
    first, stride = _Scorer.in_place([group[2]])
    assert first.data_ptr() == group[2].data_ptr() and stride is None
    for bits in ([group[0], group[1], group[3]], [group[1], group[0]], [group[0], torch.zeros(2, 5, 16, dtype=torch.uint8)],
                 [group[0], group[0]]):
        stacked, stride = _Scorer.in_place(bits)
        assert stride is None and stacked.shape == (len(bits), 2, 5, 16)
        assert stacked.data_ptr() not in {b.data_ptr() for b in bits}


def test_a_stale_library_raises_with_a_rebuild_hint(monkeypatch):
    from neurips2023_soc_amd import _lib, jf_bits
    monkeypatch.setattr(_lib, "load", lambda: object())
    with pytest.raises(_lib.SocHipError, match="soc_jf_counts_bits: a stale library .*build_ext --force"):
        jf_bits._call()
    with pytest.raises(_lib.SocHipError, match="soc_jf_bits_workspace_bytes"):
        jf_bits.workspace_bytes(1, 1, 8, 8)


def test_entry_is_declared_in_its_own_header_and_not_in_the_abi_16_set():
    import re
    from neurips2023_soc_amd import _lib, jf_bits
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "soc_hip_jf_bits.h")).read()
    declared = set(re.findall(r"^(?:int|size_t)\s+(soc_\w+)\(", hdr, re.M))
    assert declared == {jf_bits.ENTRY, jf_bits.QUERY}
    assert not declared & set(_lib.EXPORTS) and _lib.ABI_VERSION == 16
    lib = _lib.load()                                                 # loads without a GPU
    assert all(hasattr(lib, name) for name in declared)
    assert jf_bits.workspace_bytes(3, 2, 97, 130) == 3 * 5 * 97 * 3 * 8
    assert jf_bits.workspace_bytes(256, 1, 8, 8) == 0 and jf_bits.workspace_bytes(1, 0, 8, 8) == 0
    assert jf_bits.workspace_bytes(1, 1, 46341, 46341) == 0           # H * W >= 2^31


def test_cpu_tensors_are_refused():
    from neurips2023_soc_amd import _lib
    gt = torch.zeros(2, 8, 70, dtype=torch.uint8)
    with pytest.raises(_lib.SocHipError):
        RE.evaluate_video(gt, [1], torch.zeros(1, 2, 8, 16, dtype=torch.uint8))
