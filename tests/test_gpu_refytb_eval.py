"""-m gpu: K27b (soc_jf_counts_bits, include/soc_hip_jf_bits.h) against the reference-made golden, the numpy oracle of the DAVIS
tests and K27 itself, integer for integer; its workspace chunking, memory contract and argument checks; evaluate_video on the
bits K6b writes; the Ref-YouTube-VOS driver's scoring hook.  Nothing here reads the reference checkout or oracle/."""
import os

import numpy as np
import pytest
import torch

from neurips2023_soc_amd import _lib
from neurips2023_soc_amd import davis_eval as DE
from neurips2023_soc_amd import jf_bits as JB
from neurips2023_soc_amd import packed_masks as PM
from neurips2023_soc_amd import refytb_eval as RE
from neurips2023_soc_amd import synthetic_dataset as SD
from tests import guarded as G
from tests.test_gpu_davis_eval import first_difference
from tests.test_refytb_eval import GOLDEN, case_of, oracle_counts_bits

pytestmark = pytest.mark.gpu

SHAPE_CASES = ["s97x130", "s61x127", "h5_lt_r", "w6_lt_r", "h1", "w1", "p480x854", "p720x1280"]
OTHER_CASES = ["degenerate", "e1", "e5_void", "e5_novoid"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from neurips2023_soc_amd import hot_ops
    return hot_ops


def gpu_counts(gt, obj_ids, exp_obj, bits, r, use_void=True, **kw):
    as_tensor = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(a).cuda()        # noqa: E731
    return JB.jf_counts_bits(as_tensor(gt), obj_ids, exp_obj, as_tensor(bits), r, use_void, **kw)


def dirty(bits, W):
    """The same masks with every padding bit (x >= W) set."""
    every = PM.unpack(bits, bits.shape[-1] * 8).copy()
    every[..., W:] = True
    return PM.pack(every)


@pytest.mark.parametrize("c", SHAPE_CASES + OTHER_CASES)
def test_counts_equal_the_golden_and_the_oracle(ops, golden, c):
    g = golden(GOLDEN)
    gt, obj_ids, exp_obj, bits, r, use_void = case_of(g, c)
    got = gpu_counts(gt, obj_ids, exp_obj, bits, r, use_void).cpu().numpy()
    want = g[f"{c}_counts"]
    assert got.shape == want.shape == (len(exp_obj), len(gt), 6) and got.dtype == np.int32
    assert first_difference(got, want) is None, first_difference(got, want)
    oracle = oracle_counts_bits(gt, obj_ids, exp_obj, PM.unpack(bits, gt.shape[2]), r, use_void)
    assert first_difference(got, oracle) is None, first_difference(got, oracle)


def test_the_cases_cover_what_they_are_there_for(golden):
    g = golden(GOLDEN)
    assert [tuple(g[f"{c}_gt"].shape) + (int(g[f"{c}_cfg"][0]),) for c in SHAPE_CASES] == [
        (3, 97, 130, 2), (2, 61, 127, 5), (2, 5, 200, 8), (2, 150, 6, 8), (2, 1, 70, 3), (2, 70, 1, 3), (2, 480, 854, 8),
        (2, 720, 1280, 12)]
    c = g["degenerate_counts"][0]                         # n_fg / n_gt / union: empty prediction, empty truth, both, same, all
    assert c[0, 2] == 0 < c[0, 3] and c[1, 3] == 0 < c[1, 2] and c[2, 1] == 0
    assert c[3, 0] == c[3, 1] > 0 and c[4, 0] == c[4, 1] == 64 * 96 and c[5, 1] == 64 * 96 > c[5, 0]
    assert len(g["e1_exp_obj"]) == 1 and g["e5_void_exp_obj"].tolist() == [2, 0, 2, 1, 3]
    assert not (g["e5_void_gt"] == g["e5_void_obj_ids"][3]).any() and g["e5_void_counts"][4, :, 3].sum() == 0
    assert int(g["e5_void_cfg"][1]) == 1 and int(g["e5_novoid_cfg"][1]) == 0
    void = g["e5_void_gt"] == 255
    pred = PM.unpack(g["e5_void_pred_bits"], 133)
    assert (void & pred.any(0)).any() and not np.array_equal(g["e5_void_counts"][:, :, :2], g["e5_novoid_counts"][:, :, :2])


@pytest.mark.parametrize("c", ["s97x130", "e5_void", "e5_novoid", "degenerate", "p480x854"])
def test_counts_equal_k27_expression_by_expression(ops, golden, c):
    gt, obj_ids, exp_obj, bits, r, use_void = case_of(golden(GOLDEN), c)
    got = gpu_counts(gt, obj_ids, exp_obj, bits, r, use_void)
    gt_d = torch.from_numpy(gt).cuda()
    pred = PM.unpack(torch.from_numpy(bits).cuda(), gt.shape[2]).to(torch.uint8)
    for e, k in enumerate(exp_obj):
        one = torch.where(gt_d == 255, gt_d, (gt_d == obj_ids[k]).to(torch.uint8))
        k27 = ops.davis_jf_counts(one, pred[e], 1, 1, r, use_void=use_void, pairs=False)
        assert torch.equal(got[e], k27[0]), (c, e)


@pytest.mark.parametrize("c", ["s97x130", "s61x127", "h1", "w1", "w6_lt_r", "p480x854", "e5_void"])
def test_dirty_padding_bits_change_nothing(ops, golden, c):
    g = golden(GOLDEN)
    gt, obj_ids, exp_obj, bits, r, use_void = case_of(g, c)
    W = gt.shape[2]
    soiled = dirty(bits, W)
    assert W % 64 and not np.array_equal(soiled, bits) and np.array_equal(PM.unpack(soiled, W), PM.unpack(bits, W))
    got = gpu_counts(gt, obj_ids, exp_obj, soiled, r, use_void).cpu().numpy()
    assert first_difference(got, g[f"{c}_counts"]) is None, first_difference(got, g[f"{c}_counts"])


def test_predictions_cut_out_of_a_larger_buffer_are_read_in_place(ops, golden):
    g = golden(GOLDEN)
    gt, obj_ids, exp_obj, bits, r, use_void = case_of(g, "e5_void")
    E, one = len(exp_obj), bits[0].size
    front, extra = 24, 40
    buf = torch.full((E, front + one + extra), 0xFF, dtype=torch.uint8, device="cuda")             # garbage around every mask
    buf[:, front:front + one] = torch.from_numpy(bits).cuda().view(E, one)
    view = buf[:, front:front + one].view(E, *bits.shape[1:])
    assert view.stride(0) == front + one + extra > one and not view.is_contiguous()
    snapshot = buf.clone()
    with G.guarded_allocations("cuda") as served:
        got = gpu_counts(gt, obj_ids, exp_obj, view, r, use_void)
    assert len(served) == 2                                 # the workspace and the counts: no copy of the masks was made
    assert all(s.guards_intact() for s in served)
    assert first_difference(got.cpu().numpy(), g["e5_void_counts"]) is None
    # the same through the first expression's view and the distance in bytes
    again = gpu_counts(gt, obj_ids, exp_obj, view[0], r, use_void, exp_stride=view.stride(0))
    assert torch.equal(again, got) and torch.equal(buf, snapshot)
    # a slice of a group: expressions 1..3 of the five, against their own objects
    part = gpu_counts(gt, obj_ids, exp_obj[1:4], view[1:4], r, use_void)
    assert torch.equal(part, got[1:4])


def test_a_minimum_workspace_gives_the_counts_of_an_ample_one_and_runs_repeat(ops):
    T, H, W, r = 5, 97, 130, 3
    gt = SD.blob_label_maps(50, T, H, W, 2, void=True)
    pred = np.stack([SD.blob_label_maps(50, T, H, W, 2, wobble=0.03 + 0.01 * e) == k for e, k in enumerate((1, 2, 1))])
    bits, obj_ids, exp_obj = PM.pack(pred), [1, 2], [0, 1, 0]
    ample = gpu_counts(gt, obj_ids, exp_obj, bits, r)
    assert torch.equal(ample, gpu_counts(gt, obj_ids, exp_obj, bits, r))
    need = JB.workspace_bytes(3, 2, H, W)
    assert need == 3 * (2 + 3) * H * 3 * 8
    for frames in (1, 2, 5):                                # chunks of 1+1+1+1+1, 2+2+1, 5; whatever the workspace held before
        for fill in G.PATTERNS:
            ws = torch.full((need * frames + (8 if frames == 2 else 0),), fill, dtype=torch.uint8, device="cuda")
            assert torch.equal(gpu_counts(gt, obj_ids, exp_obj, bits, r, workspace=ws), ample), (frames, fill)
    want = oracle_counts_bits(gt, obj_ids, exp_obj, pred, r)
    assert first_difference(ample.cpu().numpy(), want) is None
    with pytest.raises(_lib.SocHipError, match="workspace too small|code -4"):
        gpu_counts(gt, obj_ids, exp_obj, bits, r, workspace=torch.empty(need - 8, dtype=torch.uint8, device="cuda"))


def _contract_compare(i, got, want):
    assert got.shape == want.shape and torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("c", ["s97x130", "e5_void"])
def test_memory_contract(ops, golden, c):
    """Guards around the counts, the workspace (both allocated inside the call) and both inputs; inputs unchanged; the counts
    fully written whatever the memory held (two poison patterns); the entry reached."""
    g = golden(GOLDEN)
    gt, obj_ids, exp_obj, bits, r, use_void = case_of(g, c)
    inputs = dict(gt=torch.from_numpy(gt), bits=torch.from_numpy(dirty(bits, gt.shape[2])))
    G.check_contract(inputs, lambda t: JB.jf_counts_bits(t["gt"], obj_ids, exp_obj, t["bits"], r, use_void), "cuda",
                     entry=JB.ENTRY, reference=lambda t: torch.from_numpy(g[f"{c}_counts"]), compare=_contract_compare)


def test_argument_checks_return_their_codes_without_a_launch(ops):
    import ctypes as C
    E, O, T, H, W, r = 2, 2, 2, 9, 70, 3
    RB = PM.row_bytes(W)
    one = T * H * RB
    gt = torch.zeros(T, H, W, dtype=torch.uint8, device="cuda")
    bits = torch.zeros(E * one + 8, dtype=torch.uint8, device="cuda")
    counts = torch.full((E, T, 6), -7, dtype=torch.int32, device="cuda")
    need = JB.workspace_bytes(E, O, H, W)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ints = lambda *v: (C.c_int * len(v))(*v)                  # noqa: E731
    objs, exps = ints(1, 2), ints(1, 0)
    good = dict(gt=gt.data_ptr(), bits=bits.data_ptr(), stride=one, objs=C.addressof(objs), exps=C.addressof(exps),
                counts=counts.data_ptr(), E=E, O=O, T=T, H=H, W=W, r=r, void=1, ws=ws.data_ptr(), ws_bytes=need)

    def call(**kw):
        a = {**good, **kw}
        return JB._call(a["gt"], a["bits"], a["stride"], a["objs"], a["exps"], a["counts"], a["E"], a["O"], a["T"], a["H"],
                        a["W"], a["r"], a["void"], a["ws"], a["ws_bytes"], stream)

    keep = [ints(0, 2), ints(1, 255), ints(1, 2), ints(-1, 0), ints(*([1] * 256))]
    addr = [C.addressof(k) for k in keep]
    cases = [(dict(gt=None), _lib.SOC_EINVAL), (dict(bits=None), _lib.SOC_EINVAL), (dict(objs=None), _lib.SOC_EINVAL),
             (dict(exps=None), _lib.SOC_EINVAL), (dict(counts=None), _lib.SOC_EINVAL), (dict(ws=None), _lib.SOC_EINVAL),
             (dict(E=0), _lib.SOC_EINVAL), (dict(O=0), _lib.SOC_EINVAL), (dict(T=0), _lib.SOC_EINVAL),
             (dict(H=-1), _lib.SOC_EINVAL), (dict(W=0), _lib.SOC_EINVAL),
             (dict(bits=bits.data_ptr() + 4), _lib.SOC_EINVAL), (dict(stride=one + 4), _lib.SOC_EINVAL),
             (dict(r=-1), _lib.SOC_EUNSUPPORTED), (dict(r=65), _lib.SOC_EUNSUPPORTED),
             (dict(E=256, exps=addr[4]), _lib.SOC_EUNSUPPORTED), (dict(O=256, objs=addr[4]), _lib.SOC_EUNSUPPORTED),
             (dict(objs=addr[0]), _lib.SOC_EUNSUPPORTED), (dict(objs=addr[1]), _lib.SOC_EUNSUPPORTED),
             (dict(exps=addr[2]), _lib.SOC_EUNSUPPORTED), (dict(exps=addr[3]), _lib.SOC_EUNSUPPORTED),
             (dict(H=46341, W=46341), _lib.SOC_EUNSUPPORTED), (dict(stride=one - 8), _lib.SOC_EUNSUPPORTED),
             (dict(ws_bytes=need - 1), _lib.SOC_EWORKSPACE), (dict(ws_bytes=0), _lib.SOC_EWORKSPACE)]
    for kw, code in cases:
        assert call(**kw) == code, (kw, code)
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((ws == 0xA5).all())          # nothing was launched
    assert call() == 0 and call(stride=one + 8) == 0 and call(r=0) == 0 and call(r=64) == 0
    torch.cuda.synchronize()
    assert not bool((counts == -7).any())
    with pytest.raises(_lib.SocHipError):
        JB.jf_counts_bits(gt.cpu(), [1, 2], [1, 0], bits[:E * one].view(E, T, H, RB), r)
    with pytest.raises(_lib.SocHipError, match=r"is not \[E,T,H,RB\]"):
        JB.jf_counts_bits(gt, [1, 2], [1, 0, 1], bits[:E * one].view(E, T, H, RB), r)


def test_evaluate_video_on_the_bits_k6b_writes(ops):
    """Random logits -> K6b's [E,T,H0,RB] -> evaluate_video, at the real size; the oracle sees the unpacked masks."""
    E, T, H0, W0 = 3, 2, 720, 1280
    # smooth logits (a coarse random field up-sampled twice): masks with long outlines, not salt and pepper
    coarse = torch.randn(E, T, 6, 10, generator=torch.Generator().manual_seed(11)).cuda()
    logits = torch.nn.functional.interpolate(coarse, size=(180, 320), mode="bilinear").contiguous()
    bits = PM.upsample_threshold_bits(logits, (H0, W0))
    assert bits.shape == (E, T, H0, PM.row_bytes(W0))
    gt = SD.blob_label_maps(60, T, H0, W0, 2, void=True)
    obj_ids = [1, 2, 1]
    before = JB.launches
    J, F = RE.evaluate_video(torch.from_numpy(gt).cuda(), obj_ids, bits)
    assert JB.launches == before + 1 and J.shape == F.shape == (E, T) and J.dtype == np.float64
    masks = PM.unpack(bits, W0).cpu().numpy()
    assert 0.2 < masks.mean() < 0.8
    want = oracle_counts_bits(gt, [1, 2], [0, 1, 0], masks, DE.bound_radius((H0, W0)))
    wj, wf = DE.jf_from_counts(want)
    assert np.array_equal(J, wj) and np.array_equal(F, wf)


# ---------------------------------------------------------------------------------------------------------------------
# the driver's hook

@pytest.fixture(scope="module")
def gpu_model():
    import neurips2023_soc_amd as S
    from neurips2023_soc_amd import weights as W
    model, _, _ = S.build_model(S.default_args(text_encoder_random_init=True))
    W.load_synthetic(model, 2023)
    return model.cuda().eval()


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("use_graphs,group", [(False, 1), (True, 2)])
def test_refytb_driver_scores_what_it_writes(ops, gpu_model, tmp_path, use_graphs, group, packed):
    """2 videos x 3 expressions over 2 objects: stats["jf"] and the CSVs equal refytb_eval.evaluate() run afterwards on the
    PNGs of the same call, and the PNGs are byte-identical to a run without eval_root.  The byte comparison is between two
    runs, so it uses the geometry and seed on which the DAVIS driver's test found both of its paths to repeat themselves."""
    from neurips2023_soc_amd import infer_refytb
    root = SD.make_dataset(str(tmp_path / "data"), videos=2, frames=4, height=144, width=256, expressions=3, seed=6)
    gt_root = SD.make_refytb_annotations(root, "valid", objects=2, seed=6, void=True, out_root=str(tmp_path / "gt"))
    tok = SD.HashTokenizer()
    kw = dict(size=96, max_size=160, decode_workers=2, use_graphs=use_graphs, group=group, packed_masks=packed)
    plain_dir, out_dir = str(tmp_path / "plain"), str(tmp_path / "scored")
    plain = infer_refytb.run(gpu_model, tok, root, plain_dir, **kw)
    assert "jf" not in plain and "seconds_eval" not in plain
    before = JB.launches
    stats = infer_refytb.run(gpu_model, tok, root, out_dir, eval_root=gt_root, **kw)
    # eager: one call per expression; groups of two: (v0 e0, v0 e1) (v0 e2 | v1 e0) (v1 e1, v1 e2) -- one call per video and group
    assert JB.launches - before == (4 if use_graphs else 6)
    assert stats["expressions"] == 6 and stats["seconds_eval"] > 0
    jf = stats["jf"]
    assert jf["measures"] == list(RE.G_MEASURES) and len(jf["global"]) == 7 and len(jf["per_expression"]) == 6
    _, data = infer_refytb.load_meta(root)
    for video, item in data.items():
        for exp_id in item["expressions"]:
            for name in item["frames"]:
                with open(os.path.join(out_dir, video, exp_id, name + ".png"), "rb") as x, \
                        open(os.path.join(plain_dir, video, exp_id, name + ".png"), "rb") as y:
                    assert x.read() == y.read(), (video, exp_id, name)
    csv_g, csv_e = (open(p).read() for p in RE.csv_paths(out_dir, "valid"))
    again = RE.evaluate(out_dir, gt_root, "valid")
    assert jf["global"] == again.global_row()
    assert jf["per_expression"] == [list(r) for r in again.per_expression()]
    assert (csv_g, csv_e) == RE.csv_texts(again)
    assert [r[:3] for r in jf["per_expression"]] == [[v, e, 1 + k % 2] for v in ("video000", "video001")
                                                    for k, e in enumerate(("0", "1", "2"))]


def test_scorer_refuses_ground_truth_of_another_size(ops, tmp_path):
    from neurips2023_soc_amd import infer_refytb
    root = SD.make_dataset(str(tmp_path / "small"), videos=1, frames=4, height=72, width=128, expressions=3, seed=6)
    SD.make_refytb_annotations(root, "valid", objects=2, seed=6)
    scorer = infer_refytb._Scorer(root, "valid", ["video000"], "cuda")
    try:
        scorer.begin("video000", 3)
        for shape, width in (((4, 144, PM.row_bytes(256)), 256), ((3, 72, PM.row_bytes(128)), 128), ((4, 72, PM.row_bytes(128)), 120)):
            with pytest.raises(ValueError, match=r"ground truth \(4, 72, 128\) does not match the output"):
                scorer.score("video000", ["0"], [torch.zeros(shape, dtype=torch.uint8, device="cuda")], width)
        with pytest.raises(KeyError, match="has no '7'"):
            scorer.score("video000", ["7"], [torch.zeros(4, 72, PM.row_bytes(128), dtype=torch.uint8, device="cuda")], 128)
    finally:
        scorer.reader.shutdown()


def test_command_line_scores_a_results_directory(ops, golden, tmp_path, capsys):
    from neurips2023_soc_amd import eval_refytb
    from tests.test_refytb_eval import write_tree
    g = golden(GOLDEN)
    root, results = str(tmp_path / "gt"), str(tmp_path / "runs")
    write_tree(g, root, results)
    res = RE.evaluate(results, root)
    assert res.global_row() == g["tree_global"].tolist()
    assert eval_refytb.main(["--results_path", results, "--root", root]) == 0
    paths = RE.csv_paths(results, "valid")
    assert open(paths[0]).read() == str(g["tree_csv_global"]) and open(paths[1]).read() == str(g["tree_csv_exp"])
    assert "J&F-Mean" in capsys.readouterr().out
    assert RE.evaluate(results, root, videos=["zebra"]).per_expression() == [r for r in res.per_expression() if r[0] == "zebra"]
    # --no-void and another tolerance change the numbers, not the rows
    other = RE.evaluate(results, root, use_void=False, bound_th=2)
    assert [r[:3] for r in other.per_expression()] == [r[:3] for r in res.per_expression()]
    assert other.global_row() != res.global_row()
