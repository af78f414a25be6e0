"""Per-expression J&F for the Ref-YouTube-VOS layout: every (video, expression) of a results tree against the object the
expression names, with the per-pixel work on the MI355X (K27b, jf_bits.jf_counts_bits) and the reference's f64 arithmetic
(davis_eval.jf_from_counts, db_statistics) here.  This is the protocol of a held-out part of the Ref-YouTube-VOS train
split, of Ref-DAVIS converted to the YouTube-VOS layout (the reference's davis2017/convert_davis_to_ytbs.py) and of the
MeViS valid_u kind: each expression is one row, scored over ALL listed frames.

    counts = jf_bits.jf_counts_bits(gt, obj_ids, exp_obj, pred_bits, radius)       six integers per (expression, frame)
    J, F   = evaluate_video(gt, obj_ids, pred_bits)                                [E,T] f64 each
    rows   = RefYtbJF().add(...).global_row() / .per_expression()                  the seven G_MEASURES; J-Mean, F-Mean per row

Ground truth: <root>/<split>/Annotations/<video>/<frame>.png, palette indices = object ids (255 = void), and
<root>/meta_expressions/<split>/meta_expressions.json with expressions[exp_id]["obj_id"].  Results:
<results>/<video>/<exp_id>/<frame>.png as infer_refytb writes them, pixels > 0 foreground.  The host side is numpy only.
"""
from __future__ import annotations

import csv
import io
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import davis_eval
from . import packed_masks as PM

G_MEASURES = davis_eval.G_MEASURES
EXP_MEASURES = ("Video", "Expression", "Object", "J-Mean", "F-Mean")


# ---------------------------------------------------------------------------------------------------------------------
# host side: rows and tables (numpy only)

def object_index(obj_ids_per_expression: Sequence[int]) -> Tuple[List[int], List[int]]:
    """The obj_id of each expression -> (the distinct ids, ascending; per expression its index into them): the two lists of
    K27b.  Ids outside 1..254 are refused (0 is the background, 255 void)."""
    per_exp = [int(o) for o in obj_ids_per_expression]
    for o in per_exp:
        if not 1 <= o <= 254:
            raise ValueError(f"obj_id {o} is not an object label (1..254)")
    distinct = sorted(set(per_exp))
    return distinct, [distinct.index(o) for o in per_exp]


class RefYtbJF:
    """One row per (video, expression): mean / recall / decay of J and of F over all of the video's frames
    (davis_eval.db_statistics), and the global row over the rows as DavisJF.global_row forms it.  Rows come out in sorted
    video order, then in the order the expressions were added (their order in the JSON), whatever order videos arrive in."""

    def __init__(self):
        self.rows: Dict[str, List[dict]] = {}

    def add(self, video: str, exp_id: str, obj_id: int, j_row, f_row) -> "RefYtbJF":
        jm, jr, jd = davis_eval.db_statistics(j_row)
        fm, fr, fd = davis_eval.db_statistics(f_row)
        self.rows.setdefault(str(video), []).append({"video": str(video), "exp": str(exp_id), "obj": int(obj_id),
                                                     "J": (jm, jr, jd), "F": (fm, fr, fd)})
        return self

    def add_counts(self, video: str, exp_ids: Sequence[str], obj_ids: Sequence[int], counts) -> "RefYtbJF":
        """counts [E,T,6] of one video's expressions (K27b's output, or the golden's)."""
        j, f = davis_eval.jf_from_counts(counts)
        if j.ndim != 2 or len(j) != len(exp_ids) or len(j) != len(obj_ids):
            raise ValueError(f"{video}: counts {np.shape(counts)} do not match {len(exp_ids)} expressions")
        for e, (exp_id, obj_id) in enumerate(zip(exp_ids, obj_ids)):
            self.add(video, exp_id, obj_id, j[e], f[e])
        return self

    def ordered(self) -> List[dict]:
        return [r for video in sorted(self.rows) for r in self.rows[video]]

    def global_row(self) -> List[float]:
        rows = self.ordered()
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            jm, jr, jd = ([r["J"][k] for r in rows] for k in range(3))
            fm, fr, fd = ([r["F"][k] for r in rows] for k in range(3))
            final_mean = (np.mean(jm) + np.mean(fm)) / 2.
            return [float(x) for x in (final_mean, np.mean(jm), np.mean(jr), np.mean(jd), np.mean(fm), np.mean(fr),
                                       np.mean(fd))]

    def per_expression(self) -> List[Tuple[str, str, int, float, float]]:
        return [(r["video"], r["exp"], r["obj"], float(r["J"][0]), float(r["F"][0])) for r in self.ordered()]


def csv_texts(result: RefYtbJF) -> Tuple[str, str]:
    """The text of global_results-<split>.csv (eval_davis's format) and per-expression_results-<split>.csv: header line,
    floats as %.5f, a missing value as an empty field."""
    g, s = io.StringIO(), io.StringIO()
    w = csv.writer(g, lineterminator="\n")
    w.writerow(G_MEASURES)
    w.writerow([davis_eval._fmt(x) for x in result.global_row()])
    w = csv.writer(s, lineterminator="\n")
    w.writerow(EXP_MEASURES)
    for video, exp_id, obj_id, jm, fm in result.per_expression():
        w.writerow([video, exp_id, obj_id, davis_eval._fmt(jm), davis_eval._fmt(fm)])
    return g.getvalue(), s.getvalue()


def csv_paths(results_path: str, split: str) -> Tuple[str, str]:
    return (os.path.join(results_path, f"global_results-{split}.csv"),
            os.path.join(results_path, f"per-expression_results-{split}.csv"))


def write_csvs(result: RefYtbJF, results_path: str, split: str = "valid") -> Tuple[str, str]:
    paths = csv_paths(results_path, split)
    for path, text in zip(paths, csv_texts(result)):
        with open(path, "w") as f:
            f.write(text)
    return paths


def format_tables(result: RefYtbJF, split: str) -> str:
    rows = result.per_expression()
    lines = [f"--------------------------- Global results for {split} ---------------------------",
             " ".join(f"{h:>9}" for h in G_MEASURES), " ".join(f"{davis_eval._fmt(x):>9}" for x in result.global_row()), "",
             f"---------- Per expression results for {split} ----------"]
    width = max([len(EXP_MEASURES[0])] + [len(r[0]) for r in rows])
    lines.append(f"{EXP_MEASURES[0]:>{width}} {EXP_MEASURES[1]:>10} {EXP_MEASURES[2]:>6} {EXP_MEASURES[3]:>8} {EXP_MEASURES[4]:>8}")
    lines += [f"{r[0]:>{width}} {r[1]:>10} {r[2]:>6} {davis_eval._fmt(r[3]):>8} {davis_eval._fmt(r[4]):>8}" for r in rows]
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------
# files: the ground-truth tree and a results tree

class RefYtbDataset:
    """Ground truth in the Ref-YouTube-VOS layout.  Everything that is missing is an error that names the file or key."""

    def __init__(self, root: str, split: str = "valid", videos: Optional[Sequence[str]] = None):
        self.root, self.split = root, split
        self.meta_path = os.path.join(root, "meta_expressions", split, "meta_expressions.json")
        self.mask_path = os.path.join(root, split, "Annotations")
        if not os.path.exists(self.meta_path):
            raise FileNotFoundError(f"{self.meta_path} not found")
        if not os.path.isdir(self.mask_path):
            raise FileNotFoundError(f"{self.mask_path} not found: the split has no ground-truth annotations")
        with open(self.meta_path) as f:
            self.data = json.load(f)["videos"]
        self.videos = sorted(self.data) if videos is None else sorted(str(v) for v in videos)
        for v in self.videos:
            if v not in self.data:
                raise KeyError(f"{self.meta_path}: no video '{v}'")

    def frames(self, video: str) -> List[str]:
        return list(self.data[video]["frames"])

    def expressions(self, video: str) -> List[Tuple[str, int]]:
        """(exp_id, obj_id) in the JSON's order; a split published without ground truth has no obj_id."""
        out = []
        for exp_id, item in self.data[video]["expressions"].items():
            if "obj_id" not in item:
                raise KeyError(f"{self.meta_path}: videos['{video}']['expressions']['{exp_id}'] has no 'obj_id' "
                               "(a split published without ground truth cannot be scored)")
            out.append((str(exp_id), int(item["obj_id"])))
        return out

    def masks(self, video: str) -> np.ndarray:
        """uint8 [T,H,W] label maps of the video's `frames` list (void still 255)."""
        out = []
        for frame in self.frames(video):
            path = os.path.join(self.mask_path, video, f"{frame}.png")
            if not os.path.exists(path):
                raise FileNotFoundError(f"ground-truth frame {path} not found")
            m = davis_eval._read_png(path)
            if m.ndim != 2:
                raise ValueError(f"{path}: expected a palette or grey PNG of object ids, got an array of shape {m.shape}")
            if out and m.shape != out[0].shape:
                raise ValueError(f"{path}: size {m.shape} differs from the video's first frame {out[0].shape}")
            out.append(m)
        if not out:
            raise ValueError(f"{self.meta_path}: videos['{video}']['frames'] is empty")
        return np.stack(out).astype(np.uint8)


def read_results_packed(results_path: str, video: str, exp_id: str, frames: Sequence[str], shape: Sequence[int]) -> np.ndarray:
    """The masks of one expression, packed on the host: uint8 [T,H,RB] (packed_masks.pack of `pixel > 0`).  A results tree
    with the reference's Annotations/ level (infer_refytb.py:57) is read through it."""
    base = results_path
    if not os.path.isdir(os.path.join(base, video)) and os.path.isdir(os.path.join(base, "Annotations", video)):
        base = os.path.join(base, "Annotations")
    out = np.zeros((len(frames), int(shape[0]), PM.row_bytes(int(shape[1]))), dtype=np.uint8)
    for t, frame in enumerate(frames):
        path = os.path.join(base, video, exp_id, f"{frame}.png")
        if not os.path.exists(path):
            raise FileNotFoundError(f"result frame {path} not found")
        m = davis_eval._read_png(path)
        if m.ndim == 3:                                              # an RGB(A) file: any channel set
            m = m.max(axis=2)
        if tuple(m.shape) != tuple(int(v) for v in shape):
            raise ValueError(f"{path}: size {tuple(m.shape)} does not match the ground truth {tuple(int(v) for v in shape)}")
        out[t] = PM.pack(m > 0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# device side

def video_counts(gt_labels, obj_ids: Sequence[int], pred_bits, bound_th: float = 0.008, use_void: bool = True,
                 exp_stride: Optional[int] = None):
    """gt_labels uint8 [T,H,W] and pred_bits (uint8 [E,T,H,RB], or the first expression's view with exp_stride: see
    jf_bits.jf_counts_bits) on the device; obj_ids: the obj_id of each of the E expressions -> int32 [E,T,6] on the device,
    nothing waited for."""
    from . import _lib, hot_ops, jf_bits
    hot_ops._need_gpu(gt_labels, pred_bits)
    if gt_labels.dim() != 3:
        raise _lib.SocHipError(f"expected [T,H,W] ground-truth label maps, got {tuple(gt_labels.shape)}")
    radius = davis_eval.bound_radius(tuple(gt_labels.shape[1:]), bound_th)
    if len(obj_ids) > jf_bits.MAX_IDS and pred_bits.dim() == 4:      # more expressions than one call takes: several calls
        import torch
        parts = []
        for e0 in range(0, len(obj_ids), jf_bits.MAX_IDS):
            distinct, exp_obj = object_index(obj_ids[e0:e0 + jf_bits.MAX_IDS])
            parts.append(jf_bits.jf_counts_bits(gt_labels, distinct, exp_obj, pred_bits[e0:e0 + jf_bits.MAX_IDS], radius, use_void))
        return torch.cat(parts)
    distinct, exp_obj = object_index(obj_ids)
    return jf_bits.jf_counts_bits(gt_labels, distinct, exp_obj, pred_bits, radius, use_void, exp_stride=exp_stride)


def evaluate_video(gt_labels, obj_ids: Sequence[int], pred_bits, bound_th: float = 0.008, use_void: bool = True):
    """-> (J, F), each [E,T] f64: expression e's packed masks against the object obj_ids[e] on every frame.  CPU tensors are
    refused (there is no CPU path)."""
    return davis_eval.jf_from_counts(video_counts(gt_labels, obj_ids, pred_bits, bound_th, use_void).cpu().numpy())


def evaluate(results_path: str, root: str, split: str = "valid", videos: Optional[Sequence[str]] = None,
             bound_th: float = 0.008, use_void: bool = True, device="cuda") -> RefYtbJF:
    """Scores <results_path>/<video>/<exp_id>/<frame>.png against the ground truth under `root`: one K27b call per video."""
    import torch
    dataset = RefYtbDataset(root, split, videos)
    result = RefYtbJF()
    for video in dataset.videos:
        exps = dataset.expressions(video)
        if not exps:
            continue
        gt = dataset.masks(video)
        frames = dataset.frames(video)
        bits = np.stack([read_results_packed(results_path, video, exp_id, frames, gt.shape[1:]) for exp_id, _ in exps])
        obj_ids = [o for _, o in exps]
        counts = video_counts(torch.from_numpy(gt).to(device), obj_ids, torch.from_numpy(bits).to(device), bound_th, use_void)
        result.add_counts(video, [e for e, _ in exps], obj_ids, counts.cpu().numpy())
    return result
