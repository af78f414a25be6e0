"""Writes tests/golden/refytb_jf_cases.npz: the reference's DAVIS toolkit functions (davis2017/metrics.py db_eval_iou,
f_measure, _seg2bmap; davis2017/utils.py db_statistics) run per (expression, frame) on seeded blob masks -- the per-expression
J&F protocol of refytb_eval.  Build container only: the reference checkout is not on the GPU box and nothing on the test path
reads it.

    python tests/golden/make_refytb_eval_goldens.py [--reference DIR]

The stand-ins are install_stubs of make_davis_eval_goldens.py, so the dilation primitive is the same stub by the same
definition; the six counts are formed by its counts_of and davis_eval.jf_from_counts is checked to reproduce the reference's J
and F from them before anything is written.  The reference has no per-expression script: the global row is formed here from
the reference's db_statistics with the expressions of eval_davis.py:42-46, each (video, expression) as one row, and the two
CSV texts by pandas with eval_davis.py's to_csv arguments.

Per case <c>: <c>_gt uint8 [T,H,W]; <c>_obj_ids [O]; <c>_exp_obj [E]; <c>_pred_bits uint8 [E,T,H,RB] (packed_masks.pack of
the bool masks; the width is <c>_gt's); <c>_cfg = (radius, use_void); <c>_bound_th; <c>_counts int32 [E,T,6]; <c>_J, <c>_F
f64 [E,T]; <c>_stats f64 [E,2,3] (J / F x mean, recall, decay).  The tree: tree_videos; per video <v> tree_gt_<v>,
tree_frames_<v>, tree_exps_<v> (exp ids in the JSON's order), tree_objs_<v>, tree_pred_bits_<v>, tree_counts_<v>; tree_cfg,
tree_bound_th, tree_global f64 [7], tree_rows (video, expression, object, J-Mean, F-Mean as text), tree_csv_global,
tree_csv_exp.
"""
import argparse
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_davis_eval_goldens import counts_of, install_stubs  # noqa: E402
from neurips2023_soc_amd import davis_eval, packed_masks  # noqa: E402
from neurips2023_soc_amd.synthetic_dataset import blob_label_maps  # noqa: E402


def run_case(metrics, utils, disk, dilate, gt, obj_ids, exp_obj, pred, use_void, bound_th):
    """pred bool [E,T,H,W]; expression e against the object obj_ids[exp_obj[e]]."""
    T, H, W = gt.shape
    E = len(exp_obj)
    radius = bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm((H, W)))
    J, F, C = np.zeros((E, T)), np.zeros((E, T)), np.zeros((E, T, 6), dtype=np.int32)
    for e in range(E):
        g = gt == obj_ids[exp_obj[e]]
        for t in range(T):
            v = (gt[t] == 255) if use_void else None
            J[e, t] = metrics.db_eval_iou(g[t], pred[e, t], v)
            F[e, t] = metrics.f_measure(pred[e, t], g[t], v, bound_th=bound_th)
            C[e, t] = counts_of(metrics, disk, dilate, g[t], pred[e, t], np.zeros_like(g[t]) if v is None else v, radius)
    stats = np.zeros((E, 2, 3))
    for e in range(E):
        stats[e, 0] = utils.db_statistics(J[e])
        stats[e, 1] = utils.db_statistics(F[e])
    j2, f2 = davis_eval.jf_from_counts(C)
    assert np.array_equal(j2, J) and np.array_equal(f2, F), "J / F are not reproduced from the counts"
    bits = packed_masks.pack(pred)
    assert np.array_equal(packed_masks.unpack(bits, W), pred)
    return {"gt": gt, "obj_ids": np.array(obj_ids, dtype=np.int32), "exp_obj": np.array(exp_obj, dtype=np.int32),
            "pred_bits": bits, "cfg": np.array([int(radius), int(use_void)]), "bound_th": np.float64(bound_th),
            "counts": C, "J": J, "F": F, "stats": stats}


def predictions(seed, T, H, W, objects, obj_ids, exp_obj, labels=()):
    """One bool mask stack per expression: the named object's blob, perturbed more the later the expression comes."""
    out = []
    for e, k in enumerate(exp_obj):
        maps = blob_label_maps(seed, T, H, W, max(objects, k + 1), wobble=0.03 + 0.012 * e, labels=labels)
        out.append(maps == obj_ids[k])
    return np.stack(out)


def kernel_cases():
    """name -> (gt, obj_ids, exp_obj, pred, use_void, bound_th)"""
    cases = {}

    def shape_case(name, seed, T, H, W, bound_th, void=False, objects=2, exp_obj=(0, 1, 0)):
        gt = blob_label_maps(seed, T, H, W, objects, void=void)
        obj_ids = list(range(1, objects + 1))
        cases[name] = (gt, obj_ids, list(exp_obj), predictions(seed, T, H, W, objects, obj_ids, exp_obj), int(void), bound_th)

    shape_case("s97x130", 3, 3, 97, 130, 0.008, void=True)               # r = 2, a tail of 2 bits
    shape_case("s61x127", 4, 2, 61, 127, 5)                              # r = 5 pixels, a tail of 63 bits
    shape_case("h5_lt_r", 6, 2, 5, 200, 8)                               # H < r
    shape_case("w6_lt_r", 7, 2, 150, 6, 8)                               # W < r
    shape_case("h1", 8, 2, 1, 70, 3, objects=1, exp_obj=(0, 0))
    shape_case("w1", 9, 2, 70, 1, 3, objects=1, exp_obj=(0, 0))
    shape_case("p480x854", 1, 2, 480, 854, 0.008, void=True)             # r = 8
    shape_case("p720x1280", 5, 2, 720, 1280, 0.008, void=True)           # r = 12, W a multiple of 64
    # empty prediction, empty ground truth, both empty, identical, the whole image twice, the whole image against a blob
    gt = blob_label_maps(10, 6, 64, 96, 1)
    pred = blob_label_maps(10, 6, 64, 96, 1, wobble=0.05)
    pred[0] = 0
    gt[1] = 0
    gt[2] = pred[2] = 0
    pred[3] = gt[3]
    gt[4] = pred[4] = 1
    pred[5] = 1
    cases["degenerate"] = (gt, [1], [0], (pred == 1)[None], 1, 0.008)
    # one expression
    gt = blob_label_maps(11, 3, 60, 100, 3, void=True)
    cases["e1"] = (gt, [2], [0], predictions(11, 3, 60, 100, 3, [1, 2, 3], [1])[:1], 1, 0.008)
    # five expressions over four objects with sparse labels; label 200 occurs in no frame; void on top of both masks
    labels = (7, 31, 254, 200)
    gt = blob_label_maps(12, 3, 75, 133, 3, labels=labels[:3])
    pred = predictions(12, 3, 75, 133, 4, list(labels), [2, 0, 2, 1, 3], labels=labels)
    objects_before = gt > 0
    gt[:, 20:45, 30:90] = np.where((np.indices((25, 60)).sum(0) % 7 < 3), 255, gt[:, 20:45, 30:90])   # void over gt and pred
    gt[:, 60:70, 5:40] = 255
    assert not (gt == 200).any() and pred[4].any()
    assert ((gt == 255) & pred.any(0)).any() and ((gt == 255) & objects_before).any()
    cases["e5_void"] = (gt, list(labels), [2, 0, 2, 1, 3], pred, 1, 0.008)
    cases["e5_novoid"] = (gt, list(labels), [2, 0, 2, 1, 3], pred, 0, 4)              # 255 is an ordinary label here
    return cases


def tree_videos():
    """video -> (frames, gt, [(exp_id, obj_id)] in the JSON's order, pred bool [E,T,H,W])"""
    out = {}
    gt = blob_label_maps(21, 6, 60, 100, 2, void=True)
    exps = [("2", 1), ("0", 2), ("1", 1)]                                               # not sorted: the file's order counts
    out["zebra"] = ([f"{5 * t:05d}" for t in range(6)], gt, exps, predictions(21, 6, 60, 100, 2, [1, 2], [0, 1, 0]))
    gt = blob_label_maps(22, 5, 50, 70, 2)
    exps = [("0", 2), ("1", 1), ("2", 2)]
    out["bike"] = ([f"{t:05d}" for t in range(5)], gt, exps, predictions(22, 5, 50, 70, 2, [1, 2], [1, 0, 1]))
    return out


def run_tree(metrics, utils, disk, dilate):
    import pandas as pd
    videos = tree_videos()
    out = {"videos": np.array(list(videos)), "cfg": np.array([0, 1]), "bound_th": np.float64(0.008)}
    rows, M = [], {k: [] for k in ("JM", "JR", "JD", "FM", "FR", "FD")}
    for video in sorted(videos):
        frames, gt, exps, pred = videos[video]
        obj_ids = sorted({o for _, o in exps})
        exp_obj = [obj_ids.index(o) for _, o in exps]
        res = run_case(metrics, utils, disk, dilate, gt, obj_ids, exp_obj, pred, 1, 0.008)
        out[f"gt_{video}"], out[f"frames_{video}"] = gt, np.array(frames)
        out[f"exps_{video}"], out[f"objs_{video}"] = np.array([e for e, _ in exps]), np.array([o for _, o in exps], dtype=np.int32)
        out[f"pred_bits_{video}"], out[f"counts_{video}"] = res["pred_bits"], res["counts"]
        for e, (exp_id, obj_id) in enumerate(exps):
            (jm, jr, jd), (fm, fr, fd) = res["stats"][e]
            for k, v in zip(("JM", "JR", "JD", "FM", "FR", "FD"), (jm, jr, jd, fm, fr, fd)):
                M[k].append(v)
            rows.append((video, exp_id, obj_id, jm, fm))
    final_mean = (np.mean(M["JM"]) + np.mean(M["FM"])) / 2.
    g_res = np.array([final_mean, np.mean(M["JM"]), np.mean(M["JR"]), np.mean(M["JD"]), np.mean(M["FM"]), np.mean(M["FR"]),
                      np.mean(M["FD"])])
    out["global"] = g_res
    out["rows"] = np.array([[str(x) for x in r[:3]] + [repr(float(r[3])), repr(float(r[4]))] for r in rows])
    g, s = io.StringIO(), io.StringIO()
    pd.DataFrame(data=np.reshape(g_res, [1, len(g_res)]), columns=list(davis_eval.G_MEASURES)).to_csv(
        g, index=False, float_format="%.5f")
    pd.DataFrame(data=rows, columns=["Video", "Expression", "Object", "J-Mean", "F-Mean"]).to_csv(
        s, index=False, float_format="%.5f")
    out["csv_global"], out["csv_exp"] = np.array(g.getvalue()), np.array(s.getvalue())
    return out


def main():
    from _reference_harness import REFERENCE_ROOT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REFERENCE_ROOT)
    ap.add_argument("--out", default=os.path.join(HERE, "refytb_jf_cases.npz"))
    a = ap.parse_args()
    disk, dilate = install_stubs(a.reference)
    from davis2017 import metrics, utils
    data, names = {}, []
    for name, (gt, obj_ids, exp_obj, pred, use_void, bound_th) in kernel_cases().items():
        res = run_case(metrics, utils, disk, dilate, gt, obj_ids, exp_obj, pred, use_void, bound_th)
        names.append(name)
        for k, v in res.items():
            data[f"{name}_{k}"] = v
        print(name, gt.shape, "E", len(exp_obj), "cfg", res["cfg"].tolist(), "mean J %.4f F %.4f" % (res["J"].mean(), res["F"].mean()),
              flush=True)
    data["cases"] = np.array(names)
    for k, v in run_tree(metrics, utils, disk, dilate).items():
        data[f"tree_{k}"] = v
    print("tree", data["tree_global"].tolist())
    np.savez_compressed(a.out, **data)
    size, limit = os.path.getsize(a.out), os.path.getsize(os.path.join(HERE, "davis_jf_cases.npz"))
    print(a.out, size, "bytes")
    assert size <= limit, f"{size} bytes: larger than davis_jf_cases.npz ({limit})"


if __name__ == "__main__":
    main()
