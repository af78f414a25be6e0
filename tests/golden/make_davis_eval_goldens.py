"""Writes tests/golden/davis_jf_cases.npz: the reference's DAVIS J&F toolkit (davis2017/ + eval_davis.py) run on seeded
blob label maps.  Build container only: the reference checkout is not on the GPU box and nothing on the test path reads it.

    python tests/golden/make_davis_eval_goldens.py [--reference DIR]

What runs is the reference's own code -- db_eval_iou, f_measure, _seg2bmap, the case splits, db_statistics,
DAVISEvaluation.evaluate with scipy's linear_sum_assignment, and eval_davis.py itself (as a script, through runpy) with pandas
for the two tables -- with three stand-ins for what the container lacks:
  * np.bool = bool (the numpy here no longer has the alias metrics.py uses);
  * cv2.dilate and skimage.morphology.disk, which do not exist here: the DILATION PRIMITIVE IN THESE GOLDENS IS THE STUB'S,
    BY DEFINITION -- disk(r) = {dx^2 + dy^2 <= r^2}, dilate(b, k) = scipy.ndimage.binary_dilation(b, k) with pixels outside
    the image never contributing, which is what cv2.dilate computes for a binary image and a symmetric kernel.
The six counts per (object, proposal, frame) are formed here with the reference's _seg2bmap and the same stub, following
metrics.py:29-30 and :81-97, and checked against f_measure / db_eval_iou before anything is written.

Per kernel-level case <c>: <c>_gt, <c>_pred uint8 [T,H,W]; <c>_cfg = (G, P, radius, use_void, pairs); <c>_bound_th;
<c>_counts int32 [G,P,T,6] or [G,T,6]; <c>_J, <c>_F f64 [G,P,T] or [G,T]; <c>_stats f64 [...,2,3] (J / F x mean, recall,
decay of each row).  Per tree <t>: <t>_task, <t>_seqs, <t>_gt_<seq>, <t>_res_<seq>, <t>_global f64 [7],
<t>_names, <t>_JM, <t>_FM, <t>_metrics (J / F x M / R / D per object), <t>_csv_global, <t>_csv_seq (the files' text).
"""
import argparse
import os
import runpy
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from neurips2023_soc_amd.synthetic_dataset import blob_label_maps  # noqa: E402


def install_stubs(reference_root):
    from scipy.ndimage import binary_dilation
    np.bool = bool

    def disk(radius, dtype=np.uint8):
        L = np.arange(-radius, radius + 1)
        X, Y = np.meshgrid(L, L)
        return np.array((X ** 2 + Y ** 2) <= radius ** 2, dtype=dtype)

    def dilate(src, kernel):
        return binary_dilation(src > 0, structure=kernel > 0, border_value=0).astype(np.uint8)

    cv2 = types.ModuleType("cv2")
    cv2.dilate = dilate
    skimage = types.ModuleType("skimage")
    morphology = types.ModuleType("skimage.morphology")
    morphology.disk = disk
    skimage.morphology = morphology
    sys.modules.update({"cv2": cv2, "skimage": skimage, "skimage.morphology": morphology})
    if reference_root not in sys.path:
        sys.path.insert(0, reference_root)
    return disk, dilate


def counts_of(metrics, disk, dilate, gt, fg, void, radius):
    """The six integers, with the reference's _seg2bmap and the stub dilation (metrics.py:29-30, :81-97)."""
    nv = np.logical_not(void)
    fb = metrics._seg2bmap(fg * nv)
    gb = metrics._seg2bmap(gt * nv)
    fd = dilate(fb.astype(np.uint8), disk(radius).astype(np.uint8))
    gd = dilate(gb.astype(np.uint8), disk(radius).astype(np.uint8))
    return [int(np.sum((fg & gt) & nv)), int(np.sum((fg | gt) & nv)), int(np.sum(fb)), int(np.sum(gb)),
            int(np.sum(fb * gd)), int(np.sum(gb * fd))]


def run_case(metrics, utils, disk, dilate, gt, pred, G, P, use_void, pairs, bound_th):
    T, H, W = gt.shape
    void = (gt == 255) if use_void else None
    radius = bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm((H, W)))
    shape = (G, P, T) if pairs else (G, T)
    J, F, C = np.zeros(shape), np.zeros(shape), np.zeros(shape + (6,), dtype=np.int32)
    for i in range(G):
        for j in (range(P) if pairs else [i]):
            g = gt == i + 1
            f = (pred == j + 1) if j < P else np.zeros_like(g)
            for t in range(T):
                v = None if void is None else void[t]
                jv = metrics.db_eval_iou(g[t], f[t], v)
                fv = metrics.f_measure(f[t], g[t], v, bound_th=bound_th)
                c = counts_of(metrics, disk, dilate, g[t], f[t], np.zeros_like(g[t]) if v is None else v, radius)
                idx = (i, j, t) if pairs else (i, t)
                J[idx], F[idx], C[idx] = jv, fv, c
    stats = np.zeros(shape[:-1] + (2, 3))
    for idx in np.ndindex(*shape[:-1]):
        stats[idx][0] = utils.db_statistics(J[idx])
        stats[idx][1] = utils.db_statistics(F[idx])
    # the design's premise: J and F are functions of the six counts (the product's expressions, davis_eval.jf_from_counts)
    from neurips2023_soc_amd import davis_eval
    j2, f2 = davis_eval.jf_from_counts(C)
    assert np.array_equal(j2, J) and np.array_equal(f2, F), "J / F are not reproduced from the counts"
    return {"counts": C, "J": J, "F": F, "stats": stats, "cfg": np.array([G, P, int(radius), int(use_void), int(pairs)]),
            "bound_th": np.float64(bound_th), "gt": gt, "pred": pred}


def kernel_cases():
    """name -> (gt, pred, G, P, use_void, pairs, bound_th)"""
    cases = {}

    def pair(seed, T, H, W, G, P=None, void=False, wobble=0.04):
        gt = blob_label_maps(seed, T, H, W, G, void=void)
        pred = blob_label_maps(seed, T, H, W, max(G, P or G), wobble=wobble)
        pred[pred > (P or G)] = 0
        return gt, pred

    gt, pred = pair(1, 3, 480, 854, 3, void=True)
    cases["p480x854"] = (gt, pred, 3, 3, 1, 1, 0.008)                      # r = 8, 854 = 13 * 64 + 22
    gt, pred = pair(2, 2, 480, 910, 2, void=True)
    cases["p480x910"] = (gt, pred, 2, 2, 1, 1, 0.008)                      # r = 9, 910 = 14 * 64 + 14
    gt, pred = pair(3, 3, 97, 130, 2, void=True)
    cases["s97x130"] = (gt, pred, 2, 2, 1, 1, 0.008)                       # r = 2, remainder 2
    gt, pred = pair(4, 3, 61, 127, 2)
    cases["s61x127"] = (gt, pred, 2, 2, 1, 1, 5)                           # r = 5 pixels, remainder 63
    gt, pred = pair(5, 2, 1080, 1920, 2, void=True, wobble=0.02)
    cases["p1080x1920"] = (gt, pred, 2, 2, 1, 1, 0.008)                    # r = 18: rows and words in several tiles
    gt, pred = pair(6, 3, 5, 200, 2)
    cases["h5_lt_r"] = (gt, pred, 2, 2, 1, 1, 8)                           # H < r
    gt, pred = pair(7, 3, 150, 6, 2)
    cases["w6_lt_r"] = (gt, pred, 2, 2, 1, 1, 8)                           # W < r
    gt, pred = pair(8, 2, 1, 70, 1)
    cases["h1"] = (gt, pred, 1, 1, 1, 1, 3)
    gt, pred = pair(9, 2, 70, 1, 1)
    cases["w1"] = (gt, pred, 1, 1, 1, 1, 3)
    # empty prediction, empty ground truth, both empty, identical, the whole image, whole image against a blob
    gt = blob_label_maps(10, 6, 64, 96, 1)
    pred = blob_label_maps(10, 6, 64, 96, 1, wobble=0.05)
    pred[0] = 0
    gt[1] = 0
    gt[2] = pred[2] = 0
    pred[3] = gt[3]
    gt[4] = pred[4] = 1
    pred[5] = 1
    cases["degenerate"] = (gt, pred, 1, 1, 1, 1, 0.008)
    # objects on all four borders and in the bottom-right corner, void on top of some of it
    gt = np.zeros((2, 70, 150), dtype=np.uint8)
    gt[:, :9, 20:60] = 1
    gt[:, 30:50, :7] = 2
    gt[:, -8:, 40:100] = 3
    gt[:, 10:40, -5:] = 4
    gt[:, -6:, -11:] = 5
    gt[1, -1, -1] = 0
    pred = np.roll(gt, (2, -3), axis=(1, 2))
    pred[:, -3:, -3:] = 5
    gt[:, 5:12, 50:70] = 255
    gt[:, -3:, 90:110] = 255
    cases["borders"] = (gt, pred, 5, 5, 1, 1, 0.008)
    cases["borders_r1"] = (gt, pred, 5, 5, 1, 1, 0.001)                    # ceil(0.001 * 165.5) = 1
    cases["borders_novoid"] = (gt, pred, 5, 5, 0, 1, 4)                    # 255 is an ordinary label without use_void
    gt, pred = pair(11, 3, 60, 100, 3, P=1, void=True)
    cases["g3_p1"] = (gt, pred, 3, 1, 1, 1, 0.008)
    gt, pred = pair(12, 3, 60, 100, 2, P=5, void=True)
    cases["g2_p5"] = (gt, pred, 2, 5, 1, 1, 0.008)
    gt, pred = pair(13, 2, 60, 100, 2, P=20, wobble=0.03)
    cases["g2_p20"] = (gt, pred, 2, 20, 1, 1, 0.008)
    gt, pred = pair(14, 4, 75, 133, 3, P=2, void=True)
    cases["semi_g3_p2"] = (gt, pred, 3, 2, 0, 0, 0.008)                    # prediction 3 is an empty mask
    gt, pred = pair(15, 4, 75, 133, 3)
    cases["semi_g3_p3"] = (gt, pred, 3, 3, 0, 0, 0.008)
    return cases


def tree_sequences(task):
    """name -> (gt, results): label maps of small sequences.  Proposals carry permuted labels (the assignment has to find
    them), one sequence has one proposal fewer than objects (one zero-padded row: no tie between padded rows), one has more."""
    seqs = {}
    if task == "unsupervised":
        seqs["bear"] = (blob_label_maps(21, 9, 60, 100, 3, void=True), blob_label_maps(21, 9, 60, 100, 3, wobble=0.04, labels=(2, 3, 1)))
        res = blob_label_maps(22, 7, 97, 130, 2, wobble=0.05, labels=(4, 2))
        res[:, 80:90, 5:30] = 1
        res[2:, 3:12, 100:125] = 3
        seqs["camel"] = (blob_label_maps(22, 7, 97, 130, 2, void=True), res)
        res = blob_label_maps(23, 6, 50, 70, 3, wobble=0.03, labels=(2, 0, 1))
        seqs["dog-walk"] = (blob_label_maps(23, 6, 50, 70, 3, void=True), res)
    else:
        seqs["bear"] = (blob_label_maps(31, 9, 60, 100, 3, void=True), blob_label_maps(31, 9, 60, 100, 3, wobble=0.04))
        res = blob_label_maps(32, 8, 97, 130, 3, wobble=0.05)
        res[res == 3] = 0
        seqs["camel"] = (blob_label_maps(32, 8, 97, 130, 3), res)
        seqs["dog-walk"] = (blob_label_maps(33, 6, 50, 70, 1), blob_label_maps(33, 6, 50, 70, 1, wobble=0.08))
    return seqs


def write_tree(davis_root, results_root, seqs, task):
    from PIL import Image
    os.makedirs(os.path.join(davis_root, "ImageSets", "2017"))
    with open(os.path.join(davis_root, "ImageSets", "2017", "val.txt"), "w") as f:
        f.write("".join(s + "\n" for s in seqs))
    folder = "Annotations" if task == "semi-supervised" else "Annotations_unsupervised"
    for s, (gt, res) in seqs.items():
        for d in (os.path.join(davis_root, folder, "480p", s), os.path.join(davis_root, "JPEGImages", "480p", s),
                  os.path.join(results_root, s)):
            os.makedirs(d)
        for t in range(len(gt)):
            Image.fromarray(gt[t]).save(os.path.join(davis_root, folder, "480p", s, f"{t:05d}.png"))
            Image.fromarray(res[t]).save(os.path.join(results_root, s, f"{t:05d}.png"))
            Image.fromarray(np.zeros(gt[t].shape + (3,), dtype=np.uint8)).save(
                os.path.join(davis_root, "JPEGImages", "480p", s, f"{t:05d}.jpg"))       # davis.py:48-50 wants the frames


def run_tree(reference_root, task):
    seqs = tree_sequences(task)
    out = {"task": np.array(task), "seqs": np.array(list(seqs))}
    with tempfile.TemporaryDirectory() as tmp:
        davis_root, results_root = os.path.join(tmp, "DAVIS"), os.path.join(tmp, "results")
        write_tree(davis_root, results_root, seqs, task)
        argv, sys.argv = sys.argv, ["eval_davis.py", "--davis_path", davis_root, "--set", "val", "--task", task,
                                    "--results_path", results_root]
        try:
            g = runpy.run_path(os.path.join(reference_root, "eval_davis.py"), run_name="__main__")
        finally:
            sys.argv = argv
        out["csv_global"] = np.array(open(os.path.join(results_root, "global_results-val.csv")).read())
        out["csv_seq"] = np.array(open(os.path.join(results_root, "per-sequence_results-val.csv")).read())
    res = g["metrics_res"]
    out["global"] = np.asarray(g["g_res"], dtype=np.float64)[0]
    out["names"] = np.array(g["seq_names"])
    out["JM"] = np.array(g["J_per_object"], dtype=np.float64)
    out["FM"] = np.array(g["F_per_object"], dtype=np.float64)
    out["metrics"] = np.array([[res[m][k] for k in ("M", "R", "D")] for m in ("J", "F")], dtype=np.float64)
    for s, (gt, r) in seqs.items():
        out[f"gt_{s}"], out[f"res_{s}"] = gt, r
    return out


def main():
    sys.path.insert(0, HERE)
    from _reference_harness import REFERENCE_ROOT
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REFERENCE_ROOT)
    ap.add_argument("--out", default=os.path.join(HERE, "davis_jf_cases.npz"))
    a = ap.parse_args()
    disk, dilate = install_stubs(a.reference)
    from davis2017 import metrics, utils
    data = {}
    names = []
    for name, (gt, pred, G, P, use_void, pairs, bound_th) in kernel_cases().items():
        res = run_case(metrics, utils, disk, dilate, gt, pred, G, P, use_void, pairs, bound_th)
        names.append(name)
        for k, v in res.items():
            data[f"{name}_{k}"] = v
        print(name, gt.shape, "cfg", res["cfg"].tolist(), "mean J %.4f F %.4f" % (res["J"].mean(), res["F"].mean()), flush=True)
    data["cases"] = np.array(names)
    trees = {"tree_u": "unsupervised", "tree_s": "semi-supervised"}
    for tag, task in trees.items():
        for k, v in run_tree(a.reference, task).items():
            data[f"{tag}_{k}"] = v
        print(tag, data[f"{tag}_global"].tolist(), data[f"{tag}_names"].tolist())
    data["trees"] = np.array(list(trees))
    np.savez_compressed(a.out, **data)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
