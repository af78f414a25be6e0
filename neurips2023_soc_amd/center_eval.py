"""Precision@K, overall IoU and mean IoU of the centre-frame protocol (A2D-Sentences / JHMDB-Sentences), restating the
reference's calculate_precision_at_k_and_iou_metrics (metrics.py:27-60) on the integer counts K6c gives (center_frame.py):
no mask is decoded, or even stored, to score it.

    best = select_best(scores)                      per sample, the query the reference would score
    m = metrics(counts[np.arange(N), best])         counts: int [N, 3] = (inter, pred_area, gt_area)

The arithmetic is the reference's, step by step: union = pred_area + gt_area - inter; iou = (inter + 1e-6) / (union + 1e-6)
evaluated in float32 (the reference computes it on `.float()` sums) and then widened (`.item()`); a sample counts for P@K when
iou > K; overall_iou = sum of inter / sum of union; mean_iou = the mean of the widened values.  Two empty masks give iou = 1.

Not built: the box metrics (calculate_bbox_precision_at_k_and_iou_metrics) and mAP -- mAP is pycocotools' COCOeval, which is
not available here, so no result could be checked against it.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

THRESHOLDS = (0.5, 0.6, 0.7, 0.8, 0.9)
EPS = 1e-6


def select_best(scores) -> np.ndarray:
    """scores [N, Q] -> int64 [N]: the query with the highest score; a tie goes to the LAST such query (the reference takes
    `sorted(predictions, key=score)[-1]`, and sorted is stable)."""
    s = np.asarray(scores)
    if s.ndim != 2 or s.shape[1] == 0:
        raise ValueError(f"select_best: expected scores [N, Q >= 1], got {s.shape}")
    return (s.shape[1] - 1 - np.argmax(s[:, ::-1], axis=1)).astype(np.int64)


def ious(counts) -> np.ndarray:
    """counts int [N, 3] = (inter, pred_area, gt_area) -> float64 [N]: the reference's per-sample iou (float32 arithmetic,
    widened)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    inter = c[:, 0].astype(np.float32)
    union = (c[:, 1] + c[:, 2] - c[:, 0]).astype(np.float32)
    return ((inter + np.float32(EPS)) / (union + np.float32(EPS))).astype(np.float64)


def metrics(counts) -> Dict:
    """counts int [N, 3] of the scored prediction of every sample -> {'precision_at_k': [5], 'overall_iou', 'mean_iou',
    'ious': [N], 'num_samples'}."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    if not len(c):
        raise ValueError("metrics: no samples")
    iou = ious(c)
    hits = [int(sum(1 for v in iou.tolist() if v > k)) for k in THRESHOLDS]
    inter = float(c[:, 0].astype(np.float64).sum())
    union = float((c[:, 1] + c[:, 2] - c[:, 0]).astype(np.float64).sum())
    return {"precision_at_k": (np.array(hits) / len(c)).tolist(), "overall_iou": inter / union if union else float("nan"),
            "mean_iou": float(np.mean(iou.tolist())), "ious": iou.tolist(), "num_samples": int(len(c))}


def eval_metrics(m: Dict) -> Dict:
    """The dict the reference prints (trainer.py:308-310): 'P@0.5' .. 'P@0.9', 'overall_iou', 'mean_iou'."""
    out = {f"P@{k}": p for k, p in zip(THRESHOLDS, m["precision_at_k"])}
    out.update(overall_iou=m["overall_iou"], mean_iou=m["mean_iou"])
    return out


def counts_from_masks(pred, gt) -> List[int]:
    """(inter, pred_area, gt_area) of two masks of one size (any array; non-zero = foreground): the host reference of K6c's
    counts."""
    p, g = np.asarray(pred) != 0, np.asarray(gt) != 0
    return [int((p & g).sum()), int(p.sum()), int(g.sum())]
