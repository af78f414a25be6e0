"""Host side of the DAVIS J&F evaluation (davis_eval), without a GPU: everything behind the six integer counts of K27, against
tests/golden/davis_jf_cases.npz -- the reference's davis2017/ + eval_davis.py run on seeded label maps
(tests/golden/make_davis_eval_goldens.py).  Every comparison of f64 values is `==`: the host repeats the reference's
expressions in the reference's order, so there is nothing to tolerate."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from neurips2023_soc_amd import davis_eval as DE

GOLDEN = "davis_jf_cases.npz"


def case_names(golden):
    return [str(c) for c in golden(GOLDEN)["cases"]]


def test_golden_covers_the_cases_the_kernel_is_judged_on(golden):
    g = golden(GOLDEN)
    sizes = {str(c): g[f"{c}_gt"].shape[1:] for c in g["cases"]}
    radius = {str(c): int(g[f"{c}_cfg"][2]) for c in g["cases"]}
    assert sizes["p480x854"] == (480, 854) and radius["p480x854"] == 8
    assert sizes["p480x910"] == (480, 910) and radius["p480x910"] == 9
    assert sizes["p1080x1920"] == (1080, 1920) and radius["p1080x1920"] == 18
    assert any(h < radius[c] for c, (h, w) in sizes.items()) and any(w < radius[c] for c, (h, w) in sizes.items())
    cfg = {str(c): tuple(int(v) for v in g[f"{c}_cfg"]) for c in g["cases"]}
    assert any(G > P and pairs for G, P, _, _, pairs in cfg.values())
    assert any(G < P and pairs for G, P, _, _, pairs in cfg.values())
    assert any(P == 20 for _, P, _, _, _ in cfg.values()) and any(not pairs for *_, pairs in cfg.values())


def test_jf_from_counts_equals_the_reference(golden):
    g = golden(GOLDEN)
    for c in case_names(golden):
        j, f = DE.jf_from_counts(g[f"{c}_counts"])
        assert j.dtype == np.float64 and f.dtype == np.float64
        assert np.array_equal(j, g[f"{c}_J"]), c
        assert np.array_equal(f, g[f"{c}_F"]), c


def test_jf_case_splits():
    """metrics.py:100-117: empty boundaries on either side, both, no match at all; an empty union is J = 1."""
    counts = np.array([[0, 0, 0, 0, 0, 0], [0, 9, 0, 7, 0, 0], [0, 9, 5, 0, 0, 0], [0, 9, 5, 7, 0, 0], [3, 9, 5, 7, 2, 7]])
    j, f = DE.jf_from_counts(counts)
    assert j.tolist() == [1.0, 0.0, 0.0, 0.0, 3 / 9]
    p, r = 2 / float(5), 7 / float(7)
    assert f.tolist() == [1.0, 0.0, 0.0, 0.0, 2 * p * r / (p + r)]


def test_db_statistics_equals_the_reference(golden):
    g = golden(GOLDEN)
    for c in case_names(golden):
        J, F, stats = g[f"{c}_J"], g[f"{c}_F"], g[f"{c}_stats"]
        for idx in np.ndindex(*J.shape[:-1]):
            assert list(DE.db_statistics(J[idx])) == stats[idx][0].tolist(), (c, idx)
            assert list(DE.db_statistics(F[idx])) == stats[idx][1].tolist(), (c, idx)


def test_db_statistics_bins():
    v = np.arange(10, dtype=np.float64) / 10
    m, o, d = DE.db_statistics(v)
    # four bins over round(linspace(1, 10, 5)) - 1 = 0, 2, 4, 7, 9, ends included (utils.py:151-159)
    assert (m, o, d) == (np.mean(v), 0.4, np.mean(v[0:3]) - np.mean(v[7:10]))
    # the reference's uint8 bin edges wrap past 255 frames: at 300 frames the last bin runs from 224 to 299 - 256 = 43 and is
    # empty, so its decay is nan -- reproduced, not repaired
    assert np.isnan(DE.db_statistics(np.linspace(0, 1, 300))[2])
    assert not np.isnan(DE.db_statistics(np.linspace(0, 1, 200))[2])


def test_bound_radius():
    assert [DE.bound_radius(s) for s in ((480, 854), (480, 910), (720, 1280), (1080, 1920), (97, 130))] == [8, 9, 12, 18, 2]
    assert DE.bound_radius((10, 10), 3) == 3 and DE.bound_radius((10, 10), 4.0) == 4
    with pytest.raises(ValueError, match="whole number"):
        DE.bound_radius((10, 10), 2.5)


def brute_force(cost):
    nr, nc = cost.shape
    best, best_val = None, np.inf
    if nr <= nc:
        for cols in itertools.permutations(range(nc), nr):
            val = sum(cost[i, c] for i, c in enumerate(cols))
            if val < best_val:
                best, best_val = (list(range(nr)), list(cols)), val
    else:
        for rows in itertools.permutations(range(nr), nc):
            val = sum(cost[r, j] for j, r in enumerate(rows))
            if val < best_val:
                order = np.argsort(rows)
                best, best_val = ([rows[k] for k in order], [int(k) for k in order]), val
    return best


def test_assign_against_brute_force():
    """Seeded continuous costs: the optimum is unique (which optimum is returned under ties is unspecified)."""
    rng = np.random.default_rng(0)
    for nr in range(1, 7):
        for nc in range(1, 7):
            cost = rng.normal(size=(nr, nc))
            rows, cols = DE.assign(cost)
            assert (rows.tolist(), cols.tolist()) == tuple(brute_force(cost)), (nr, nc)
            assert rows.tolist() == sorted(rows.tolist()) and len(rows) == min(nr, nc)
    assert [x.tolist() for x in DE.assign(np.zeros((0, 3)))] == [[], []]
    with pytest.raises(ValueError):
        DE.assign(np.array([[np.nan, 1.0]]))


def test_assign_against_scipy():
    """Continuous seeded costs, no ties (tie-breaking is unspecified in both); up to the sizes the evaluation can meet."""
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(1)
    for nr, nc in ((20, 20), (20, 7), (7, 20), (20, 255), (255, 20), (3, 1), (1, 3), (40, 40)):
        cost = -rng.uniform(size=(nr, nc))
        rows, cols = DE.assign(cost)
        want_rows, want_cols = lsa(cost)
        assert np.array_equal(rows, want_rows) and np.array_equal(cols, want_cols), (nr, nc)


def test_unsupervised_rows_come_in_proposal_order():
    """evaluation.py:63-64 indexes the scores by (row_ind, col_ind) with row_ind the PROPOSALS in ascending order, and
    evaluate() names row k <seq>_<k+1>: with proposal 1 matching object 2 and proposal 2 matching object 1, "<seq>_1" carries
    object 2's score."""
    T = 3
    counts = np.zeros((2, 2, T, 6), dtype=np.int32)            # [object, proposal, frame]
    counts[0, 1] = [9, 10, 4, 4, 4, 4]                         # object 1 <-> proposal 2: J = 0.9
    counts[1, 0] = [5, 10, 4, 4, 2, 2]                         # object 2 <-> proposal 1: J = 0.5
    counts[0, 0] = counts[1, 1] = [0, 10, 4, 4, 0, 0]
    j_rows, f_rows = DE.sequence_measures(counts, "unsupervised")
    assert j_rows[:, 0].tolist() == [0.5, 0.9] and f_rows[:, 0].tolist() == [0.5, 1.0]
    res = DE.DavisJF().add("seq", j_rows, f_rows)
    assert res.per_sequence() == [("seq_1", 0.5, 0.5), ("seq_2", 0.9, 1.0)]
    with pytest.raises(ValueError, match="P >= G"):
        DE.sequence_measures(counts[:, :1], "unsupervised")


def golden_tree_counts(g, tag):
    """Counts of a golden tree's sequences from the numpy oracle of the GPU test file (bool arrays, explicit loops): the CPU
    stand-in for K27 here, so that aggregation and CSV text are checked end to end without a GPU."""
    from tests.test_gpu_davis_eval import oracle_counts
    task = str(g[f"{tag}_task"])
    out = {}
    for s in g[f"{tag}_seqs"]:
        gt, res = g[f"{tag}_gt_{s}"], g[f"{tag}_res_{s}"]
        G = int(np.where(gt[0] == 255, 0, gt[0]).max())
        if task == "semi-supervised":
            gt, res = gt[1:-1], res[1:-1]
            P = int(res.max())
            out[str(s)] = oracle_counts(gt, res, G, P, DE.bound_radius(gt.shape[1:]), use_void=False, pairs=False)
        else:
            P = max(int(res.max()), G)
            out[str(s)] = oracle_counts(gt, res, G, P, DE.bound_radius(gt.shape[1:]), use_void=True, pairs=True)
    return task, out


@pytest.mark.parametrize("tag", ["tree_u", "tree_s"])
def test_tables_and_csv_text_equal_the_reference(golden, tag, tmp_path):
    g = golden(GOLDEN)
    task, counts = golden_tree_counts(g, tag)
    res = DE.DavisJF()
    for s, c in counts.items():
        res.add(s, *DE.sequence_measures(c, task))
    assert res.global_row() == g[f"{tag}_global"].tolist()
    table = res.per_sequence()
    assert [r[0] for r in table] == [str(n) for n in g[f"{tag}_names"]]
    assert [r[1] for r in table] == g[f"{tag}_JM"].tolist() and [r[2] for r in table] == g[f"{tag}_FM"].tolist()
    for a, m in enumerate(("J", "F")):
        for b, k in enumerate(("M", "R", "D")):
            assert [float(x) for x in res.metrics_res[m][k]] == g[f"{tag}_metrics"][a, b].tolist(), (m, k)
    paths = DE.write_csvs(res, str(tmp_path), "val")
    assert [p.split("/")[-1] for p in paths] == ["global_results-val.csv", "per-sequence_results-val.csv"]
    assert open(paths[0]).read() == str(g[f"{tag}_csv_global"])
    assert open(paths[1]).read() == str(g[f"{tag}_csv_seq"])


def test_oracle_counts_equal_the_golden_counts(golden):
    """The numpy oracle the GPU test uses beyond the golden cases is itself pinned to the reference here (small cases)."""
    from tests.test_gpu_davis_eval import oracle_counts
    g = golden(GOLDEN)
    for c in case_names(golden):
        gt = g[f"{c}_gt"]
        if gt[0].size > 20000:
            continue
        G, P, r, use_void, pairs = (int(v) for v in g[f"{c}_cfg"])
        assert np.array_equal(oracle_counts(gt, g[f"{c}_pred"], G, P, r, bool(use_void), bool(pairs)), g[f"{c}_counts"]), c


def test_entry_point_decides_argument_errors_from_the_sizes():
    """soc_davis_jf_counts_u8 refuses bad arguments before any launch (the pointers are never dereferenced): no GPU needed."""
    from neurips2023_soc_amd import _lib, build_ext
    build_ext.build(verbose=False)
    lib = _lib.load()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    G, P, T, H, W = 2, 3, 4, 48, 100
    need = lib.soc_davis_jf_workspace_bytes(G, P, T, H, W)
    assert need == T * (G + P) * H * 2 * 8 * 3            # three one-bit planes of ceil(100 / 64) words per row

    def call(gt=p, pred=p, counts=p, G=G, P=P, T=T, H=H, W=W, radius=8, ws=p, ws_bytes=need):
        return lib.soc_davis_jf_counts_u8(gt, pred, counts, G, P, T, H, W, radius, 1, 1, ws, ws_bytes, None)

    for kw in ({"gt": None}, {"pred": None}, {"counts": None}, {"ws": None}, {"T": 0}, {"H": 0}, {"W": -1}):
        assert call(**kw) == _lib.SOC_EINVAL, kw
    for kw in ({"radius": -1}, {"radius": 65}, {"G": 256}, {"P": 256}, {"G": -1}, {"P": -1}, {"G": 0, "P": 0}):
        assert call(**kw) == _lib.SOC_EUNSUPPORTED, kw
    assert call(ws_bytes=need - 1) == _lib.SOC_EWORKSPACE
    assert lib.soc_davis_jf_workspace_bytes(0, 0, T, H, W) == 0 and lib.soc_davis_jf_workspace_bytes(G, P, T, 0, W) == 0
    # whole sequences at 1080p with every proposal slot used stay within a bounded workspace (frames go through in chunks)
    assert 0 < lib.soc_davis_jf_workspace_bytes(10, 20, 100, 1080, 1920) <= 128 << 20


def test_cpu_tensors_are_refused():
    from neurips2023_soc_amd import hot_ops
    x = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hot_ops.davis_jf_counts(x, x, 1, 1, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DE.evaluate_sequence(x, x, "unsupervised", num_objects=1)


def test_sequence_errors_carry_the_reference_messages(monkeypatch):
    from neurips2023_soc_amd import hot_ops
    monkeypatch.setattr(hot_ops, "davis_jf_counts", lambda *a, **k: pytest.fail("refused before any launch"))
    gt = torch.zeros(4, 8, 8, dtype=torch.uint8)
    gt[:, 2:4, 2:4] = 1
    pred = gt.clone()
    pred[2, 5, 5] = 21
    with pytest.raises(ValueError, match=r"maximum number \(20\) of proposals allowed"):
        DE.evaluate_sequence(gt, pred, "unsupervised")
    with pytest.raises(ValueError, match="higher than the number of objects in the sequence"):
        DE.evaluate_sequence(gt, pred, "semi-supervised")
    with pytest.raises(ValueError, match="one size"):
        DE.evaluate_sequence(gt, pred[:3], "unsupervised")


def test_missing_result_frame_and_missing_tree(tmp_path):
    with pytest.raises(FileNotFoundError, match="DAVIS not found"):
        DE.DavisDataset(str(tmp_path / "nope"))
    with pytest.raises(FileNotFoundError, match="bear frame 00000 not found!"):
        DE.read_results(str(tmp_path), "bear", ["00000"])


def test_synthetic_annotations_layout(tmp_path):
    from neurips2023_soc_amd import synthetic_dataset as SD
    root = SD.make_dataset(str(tmp_path / "data"), videos=2, frames=3, height=48, width=80, expressions=8, seed=5)
    davis = SD.make_davis_annotations(root, str(tmp_path / "DAVIS"), objects=2, void=True, seed=5)
    for task in DE.TASKS:
        ds = DE.DavisDataset(davis, task)
        assert ds.sequences == ["video000", "video001"]
        maps, ids = ds.masks("video001")
        assert maps.shape == (3, 48, 80) and maps.dtype == np.uint8 and ids == ["00000", "00001", "00002"]
        assert set(np.unique(maps)) == {0, 1, 2, 255}
    again = SD.blob_label_maps(5 * 1000 + 1, 3, 48, 80, 2, void=True)
    assert np.array_equal(maps, again)
