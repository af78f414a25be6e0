"""DAVIS J&F evaluation: what the reference's eval_davis.py + davis2017/ compute from PNG label maps, with the per-pixel
work on the MI355X (K27, hot_ops.davis_jf_counts) and the reference's float arithmetic, in the reference's order, here.

    counts = hot_ops.davis_jf_counts(gt, pred, G, P, radius)      six integers per (object, proposal, frame)
    J, F   = jf_from_counts(counts)                               davis2017/metrics.py:32-36, :99-117
    M R D  = db_statistics(per-frame values)                      davis2017/utils.py:135-161
    rows   = DavisJF().add(...).global_row() / .per_sequence()    davis2017/evaluation.py:66-110, eval_davis.py:39-60

Because the device only produces integers and everything after them is the same f64 expression the reference evaluates,
the numbers equal the reference toolkit's on the same masks, to the last digit.  numpy only (no scipy, no pandas): the
assignment of proposals to objects (task "unsupervised") is the small solver `assign` below.
"""
from __future__ import annotations

import csv
import glob
import io
import os
import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np

TASKS = ("semi-supervised", "unsupervised")
SUBSETS = ("train", "val", "test-dev", "test-challenge")
VOID_LABEL = 255
MAX_PROPOSALS = 20
G_MEASURES = ("J&F-Mean", "J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay")
SEQ_MEASURES = ("Sequence", "J-Mean", "F-Mean")
DATASET_WEB = "https://davischallenge.org/davis2017/code.html"


def bound_radius(shape: Sequence[int], bound_th: float = 0.008) -> int:
    """Radius in pixels of the boundary tolerance disk (metrics.py:77-78): bound_th itself when >= 1 (a whole number of
    pixels), otherwise ceil(bound_th * |(H, W)|_2) in f64 -- 8 at 480x854, 12 at 720p, 18 at 1080p."""
    if bound_th >= 1:
        if bound_th != int(bound_th):
            raise ValueError(f"bound_th >= 1 is a radius in pixels and must be a whole number, got {bound_th}")
        return int(bound_th)
    return int(np.ceil(bound_th * np.linalg.norm(tuple(int(v) for v in shape))))


def jf_from_counts(counts) -> Tuple[np.ndarray, np.ndarray]:
    """[..., 6] integer counts (inter, union, n_fg, n_gt, fg_match, gt_match) -> (J, F), f64 arrays of shape [...].
    J = inter / union, 1 where the union is empty (metrics.py:32-36).  F: precision = fg_match / n_fg, recall =
    gt_match / n_gt, with the reference's case split for empty boundaries (:100-111), F = 2 p r / (p + r), 0 where
    p + r == 0 (:114-117)."""
    c = np.asarray(counts).astype(np.int64)
    inter, union, n_fg, n_gt, fg_match, gt_match = (c[..., k] for k in range(6))
    with np.errstate(divide="ignore", invalid="ignore"):
        j = inter / union
        j = np.where(union == 0, 1.0, j)
        precision = np.where(n_fg == 0, 1.0, np.where(n_gt == 0, 0.0, fg_match / n_fg.astype(np.float64)))
        recall = np.where(n_gt == 0, 1.0, np.where(n_fg == 0, 0.0, gt_match / n_gt.astype(np.float64)))
        f = np.where(precision + recall == 0, 0.0, 2 * precision * recall / (precision + recall))
    return j, f


def db_statistics(per_frame_values) -> Tuple[float, float, float]:
    """(mean, recall, decay) of one object's per-frame values (utils.py:135-161): mean, share of frames > 0.5, and the
    mean of the first minus the mean of the last of four bins.  The bin edges pass through uint8 as in the reference, so
    sequences of more than 256 frames wrap the same way."""
    v = np.asarray(per_frame_values, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        m = np.nanmean(v)
        o = np.nanmean(v > 0.5)
        ids = np.round(np.linspace(1, len(v), 5) + 1e-10) - 1
        ids = ids.astype(np.uint8)
        d = np.nanmean(v[ids[0]:ids[1] + 1]) - np.nanmean(v[ids[3]:ids[4] + 1])
    return m, o, d


def assign(cost) -> Tuple[np.ndarray, np.ndarray]:
    """Rectangular linear sum assignment, minimising: (row_ind, col_ind) with row_ind ascending, min(rows, cols) pairs -- the
    interface of scipy.optimize.linear_sum_assignment, which evaluation.py:63 calls.  Shortest augmenting paths with dual
    variables (Jonker-Volgenant as restated by Crouse, 2016); sizes here are <= 255 x <= 255.  Which of several optimal
    assignments is returned when costs tie is unspecified, here as there."""
    cost = np.array(cost, dtype=np.float64)
    if cost.ndim != 2:
        raise ValueError("expected a matrix")
    if cost.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    if not np.all(np.isfinite(cost)):
        raise ValueError("matrix contains invalid numeric entries")
    transposed = cost.shape[1] < cost.shape[0]
    if transposed:
        cost = cost.T
    nr, nc = cost.shape
    u, v = np.zeros(nr), np.zeros(nc)
    path = np.full(nc, -1)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    for cur in range(nr):
        shortest = np.full(nc, np.inf)
        in_sr, in_sc = np.zeros(nr, dtype=bool), np.zeros(nc, dtype=bool)
        remaining = list(range(nc - 1, -1, -1))
        min_val, i, sink = 0.0, cur, -1
        while sink == -1:
            index, lowest = -1, np.inf
            in_sr[i] = True
            for it, j in enumerate(remaining):
                r = min_val + cost[i, j] - u[i] - v[j]
                if r < shortest[j]:
                    path[j] = i
                    shortest[j] = r
                if shortest[j] < lowest or (shortest[j] == lowest and row4col[j] == -1):
                    lowest = shortest[j]
                    index = it
            min_val = lowest
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            in_sc[j] = True
            remaining[index] = remaining[-1]
            remaining.pop()
        u[cur] += min_val
        for i in range(nr):
            if in_sr[i] and i != cur:
                u[i] += min_val - shortest[col4row[i]]
        for j in range(nc):
            if in_sc[j]:
                v[j] -= min_val - shortest[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if transposed:
        order = np.argsort(col4row)
        return col4row[order].astype(np.int64), order.astype(np.int64)
    return np.arange(nr, dtype=np.int64), col4row.astype(np.int64)


def sequence_measures(counts, task: str) -> Tuple[np.ndarray, np.ndarray]:
    """Counts of one sequence -> (J, F), each [objects, frames] f64, one row per evaluated object.
    "semi-supervised": counts [G,T,6], row k is object k + 1 (evaluation.py:35-41).
    "unsupervised": counts [G,P,T,6] with P >= G; every (proposal, object) pair is scored and the pairs that maximise the
    mean over frames of (J + F) / 2 are kept (:51-64).  The reference indexes the result by the assignment's row index,
    which is the PROPOSAL, sorted ascending -- so row k of the output is the k-th smallest assigned proposal, not object
    k + 1, and the per-object names are attached in that order (:91-104).  Reproduced."""
    if task not in TASKS:
        raise ValueError(f"The only tasks that are supported are {list(TASKS)}")
    j, f = jf_from_counts(counts)
    if task == "semi-supervised":
        if j.ndim != 2:
            raise ValueError("semi-supervised counts are [G,T,6]")
        return j, f
    if j.ndim != 3 or j.shape[1] < j.shape[0]:
        raise ValueError("unsupervised counts are [G,P,T,6] with P >= G (missing proposals are empty masks)")
    j = np.ascontiguousarray(j.transpose(1, 0, 2))          # [proposal, object, frame], the reference's layout: same sums
    f = np.ascontiguousarray(f.transpose(1, 0, 2))
    all_metrics = (np.mean(j, axis=2) + np.mean(f, axis=2)) / 2
    row_ind, col_ind = assign(-all_metrics)
    return j[row_ind, col_ind, :], f[row_ind, col_ind, :]


class DavisJF:
    """Accumulates sequences into the reference's `metrics_res` structure (evaluation.py:74-104) and forms the two tables
    of eval_davis.py:39-60."""

    def __init__(self):
        self.metrics_res = {m: {"M": [], "R": [], "D": [], "M_per_object": {}} for m in ("J", "F")}

    def add(self, seq: str, j_rows, f_rows) -> "DavisJF":
        for ii in range(len(j_rows)):
            name = f"{seq}_{ii + 1}"
            for key, rows in (("J", j_rows), ("F", f_rows)):
                m, r, d = db_statistics(rows[ii])
                res = self.metrics_res[key]
                res["M"].append(m)
                res["R"].append(r)
                res["D"].append(d)
                res["M_per_object"][name] = m
        return self

    def global_row(self) -> List[float]:
        J, F = self.metrics_res["J"], self.metrics_res["F"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            final_mean = (np.mean(J["M"]) + np.mean(F["M"])) / 2.
            return [float(x) for x in (final_mean, np.mean(J["M"]), np.mean(J["R"]), np.mean(J["D"]), np.mean(F["M"]),
                                       np.mean(F["R"]), np.mean(F["D"]))]

    def per_sequence(self) -> List[Tuple[str, float, float]]:
        J, F = self.metrics_res["J"], self.metrics_res["F"]
        return [(name, float(J["M_per_object"][name]), float(F["M_per_object"][name])) for name in J["M_per_object"]]


def _fmt(x: float) -> str:
    return "" if x != x else "%.5f" % x          # pandas writes a missing value as an empty field


def csv_texts(result: DavisJF) -> Tuple[str, str]:
    """The text of global_results-<set>.csv and per-sequence_results-<set>.csv: header line, no index column, floats as
    %.5f -- what DataFrame.to_csv(index=False, float_format="%.5f") writes for the tables of eval_davis.py:42-59."""
    g, s = io.StringIO(), io.StringIO()
    w = csv.writer(g, lineterminator="\n")
    w.writerow(G_MEASURES)
    w.writerow([_fmt(x) for x in result.global_row()])
    w = csv.writer(s, lineterminator="\n")
    w.writerow(SEQ_MEASURES)
    for name, jm, fm in result.per_sequence():
        w.writerow([name, _fmt(jm), _fmt(fm)])
    return g.getvalue(), s.getvalue()


def csv_paths(results_path: str, gt_set: str) -> Tuple[str, str]:
    return (os.path.join(results_path, f"global_results-{gt_set}.csv"),
            os.path.join(results_path, f"per-sequence_results-{gt_set}.csv"))


def write_csvs(result: DavisJF, results_path: str, gt_set: str = "val") -> Tuple[str, str]:
    paths = csv_paths(results_path, gt_set)
    for path, text in zip(paths, csv_texts(result)):
        with open(path, "w") as f:
            f.write(text)
    return paths


# ---------------------------------------------------------------------------------------------------------------------
# device side: label maps -> counts -> per-object rows

def count_objects(gt_labels) -> int:
    """Objects of a sequence: the largest label of the FIRST ground-truth frame, void excluded (davis.py:88-93)."""
    first = gt_labels[0]
    return int(first.masked_fill(first == VOID_LABEL, 0).max())


def evaluate_sequence(gt_labels, pred_labels, task: str = "unsupervised", bound_th: float = 0.008,
                      num_objects: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """gt_labels, pred_labels: uint8 [T,H,W] tensors on the device (label maps as the PNGs hold them; 255 in gt = void)
    -> (J, F) rows per object as sequence_measures returns them; DavisJF.add / db_statistics give M / R / D.
    "semi-supervised": first and last frame dropped, void not used, prediction k against object k; more predicted objects
    than the sequence has is an error.  "unsupervised": all frames, void applied to J and F, at most 20 proposals.
    The messages of the two errors are the reference's (evaluation.py:30, :46), which exits there."""
    from . import hot_ops
    if task not in TASKS:
        raise ValueError(f"The only tasks that are supported are {list(TASKS)}")
    if tuple(gt_labels.shape) != tuple(pred_labels.shape) or gt_labels.dim() != 3:
        raise ValueError(f"ground truth {tuple(gt_labels.shape)} and result {tuple(pred_labels.shape)} label maps must be "
                         "[T,H,W] of one size")
    G = count_objects(gt_labels) if num_objects is None else int(num_objects)
    if task == "semi-supervised":
        gt_labels, pred_labels = gt_labels[1:-1], pred_labels[1:-1]
    T, H, W = gt_labels.shape
    if T == 0:
        raise ValueError("no frames to evaluate")
    P = int(pred_labels.max())
    if G == 0:
        return np.zeros((0, T)), np.zeros((0, T))
    radius = bound_radius((H, W), bound_th)
    if task == "semi-supervised":
        if P > G:
            raise ValueError("In your PNG files there is an index higher than the number of objects in the sequence!")
        counts = hot_ops.davis_jf_counts(gt_labels, pred_labels, G, P, radius, use_void=False, pairs=False)
    else:
        if P > MAX_PROPOSALS:
            raise ValueError(f"In your PNG files there is an index higher than the maximum number ({MAX_PROPOSALS}) of "
                             "proposals allowed!")
        counts = hot_ops.davis_jf_counts(gt_labels, pred_labels, G, max(P, G), radius, use_void=True, pairs=True)
    return sequence_measures(counts.cpu().numpy(), task)


# ---------------------------------------------------------------------------------------------------------------------
# files: the DAVIS tree and a results tree (davis2017/davis.py, davis2017/results.py)

def _read_png(path: str) -> np.ndarray:
    from PIL import Image
    return np.array(Image.open(path))


class DavisDataset:
    """Ground truth of a DAVIS tree: ImageSets/<year>/<set>.txt and Annotations[_unsupervised]/480p/<seq>/*.png
    (davis.py:14-63).  The frames of a sequence are its annotation PNGs, sorted; JPEGImages is not read."""

    def __init__(self, root: str, task: str = "unsupervised", subset: str = "val", sequences="all",
                 resolution: str = "480p"):
        if subset not in SUBSETS:
            raise ValueError(f"Subset should be in {list(SUBSETS)}")
        if task not in TASKS:
            raise ValueError(f"The only tasks that are supported are {list(TASKS)}")
        self.root, self.task, self.subset = root, task, subset
        self.mask_path = os.path.join(root, "Annotations" if task == "semi-supervised" else "Annotations_unsupervised",
                                      resolution)
        year = "2019" if task == "unsupervised" and subset in ("test-dev", "test-challenge") else "2017"
        listing = os.path.join(root, "ImageSets", year, f"{subset}.txt")
        if not os.path.exists(root):
            raise FileNotFoundError(f"DAVIS not found in the specified directory, download it from {DATASET_WEB}")
        if not os.path.exists(listing):
            raise FileNotFoundError(f"Subset sequences list for {subset} not found, download the missing subset "
                                    f"for the {task} task from {DATASET_WEB}")
        if not os.path.exists(self.mask_path):
            raise FileNotFoundError(f"Annotations folder for the {task} task not found, download it from {DATASET_WEB}")
        if sequences == "all":
            with open(listing) as f:
                self.sequences = [x.strip() for x in f.readlines() if x.strip()]
        else:
            self.sequences = list(sequences) if isinstance(sequences, (list, tuple)) else [sequences]

    def masks(self, seq: str) -> Tuple[np.ndarray, List[str]]:
        """uint8 [T,H,W] label maps (void still 255) and the frame ids (file names without .png)."""
        paths = sorted(glob.glob(os.path.join(self.mask_path, seq, "*.png")))
        if not paths:
            raise FileNotFoundError(f"Annotations for sequence {seq} not found.")
        ids = [os.path.splitext(os.path.basename(p))[0] for p in paths]
        return np.stack([_read_png(p) for p in paths]).astype(np.uint8), ids


def read_results(results_path: str, seq: str, ids: Sequence[str]) -> np.ndarray:
    """Result label maps of the given frames (results.py:11-26); a missing frame is a FileNotFoundError with the
    reference's message."""
    out = []
    for frame_id in ids:
        path = os.path.join(results_path, seq, f"{frame_id}.png")
        try:
            out.append(_read_png(path))
        except IOError as err:
            raise FileNotFoundError(f"{seq} frame {frame_id} not found!\nThe frames have to be indexed PNG files placed "
                                    "inside the corespondent sequence folder.\nThe indexes have to match with the initial "
                                    "frame.\n") from err
    return np.stack(out).astype(np.uint8)


def evaluate(results_path: str, davis_path: str, task: str = "unsupervised", gt_set: str = "val", sequences="all",
             device="cuda", bound_th: float = 0.008) -> DavisJF:
    """The reference's DAVISEvaluation(davis_path, task, gt_set, sequences).evaluate(results_path), metric ('J', 'F')."""
    import torch
    dataset = DavisDataset(davis_path, task, gt_set, sequences)
    result = DavisJF()
    for seq in dataset.sequences:
        gt, ids = dataset.masks(seq)
        # the semi-supervised task reads only the frames it scores (evaluation.py:84-86); evaluate_sequence drops the
        # two ends itself, so they are filled with background here
        res = read_results(results_path, seq, ids[1:-1] if task == "semi-supervised" else ids)
        if task == "semi-supervised":
            pad = np.zeros((1,) + res.shape[1:], dtype=np.uint8)
            res = np.concatenate([pad, res, pad]) if len(res) else res
        if res.shape != gt.shape:
            raise ValueError(f"{seq}: result label maps {res.shape} do not match the ground truth {gt.shape}")
        j_rows, f_rows = evaluate_sequence(torch.from_numpy(gt).to(device), torch.from_numpy(res).to(device), task, bound_th)
        result.add(seq, j_rows, f_rows)
    return result


def mean_rows(rows: Sequence[Sequence[float]]) -> List[float]:
    """Column means of several global rows (the figure Ref-DAVIS papers quote is the mean over the four annotators)."""
    return [float(x) for x in np.mean(np.asarray(rows, dtype=np.float64), axis=0)]


def format_tables(global_row: Sequence, per_sequence: Sequence[Sequence], gt_set: str) -> str:
    def cell(x):
        return x if isinstance(x, str) else _fmt(x)
    lines = [f"--------------------------- Global results for {gt_set} ---------------------------",
             " ".join(f"{h:>9}" for h in G_MEASURES), " ".join(f"{cell(x):>9}" for x in global_row), "",
             f"---------- Per sequence results for {gt_set} ----------"]
    width = max([len(SEQ_MEASURES[0])] + [len(str(r[0])) for r in per_sequence])
    lines.append(f"{SEQ_MEASURES[0]:>{width}} {SEQ_MEASURES[1]:>8} {SEQ_MEASURES[2]:>8}")
    lines += [f"{r[0]:>{width}} {cell(r[1]):>8} {cell(r[2]):>8}" for r in per_sequence]
    return "\n".join(lines)
