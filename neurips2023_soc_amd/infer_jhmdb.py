"""JHMDB-Sentences evaluation driver: the reference's centre-frame protocol (trainer.py:253-313 over
datasets/jhmdb_sentences/jhmdb_sentences_dataset.py) on the MI355X pipeline.

    for each sample (video, annotated frame, query)                    dataset :91-142
      the 8-frame window around the frame, edge frames repeated        :96-105    decoded, then K9 on the GPU (320 / 576)
      forward with valid_indices = the window's centre                 trainer.py:262-275   Video-Swin on 8 frames, the rest on 1
      masks of all queries at the original size, counts against the ground truth      ONE K6c launch per batch of samples
    P@K, overall IoU, mean IoU from the counts of each sample's best-scored query      center_eval (metrics.py:27-60)

Dataset layout (dataset :44-81): <root>/jhmdb_annotation.txt (CSV: video_id,query under a header line),
<root>/Rename_Images/<action>/<video>/%05d.png (1-indexed) and <root>/puppet_mask/<action>/<video>/puppet_mask.mat with
`part_mask` [H, W, frames]; frames beyond the number of masks are ignored.  The samples -- three annotated frames per (video,
query) -- come from a samples file in the reference's metadata format (rows of [video_id, frame_path, masks_path,
total_frames, query]; only the frame number of frame_path is used) or are drawn here and written to <out>/samples.json.

Not built: the A2D-Sentences reader (mp4 + HDF5), mAP and compressed RLE strings (both pycocotools).
"""
from __future__ import annotations

import csv
import glob
import json
import os
import random
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import center_eval, center_frame, clip_io
from .infer_refytb import Tokenize
from .nested_tensor import NestedTensor

WINDOW = 8
FRAMES_PER_QUERY = 3
PAD_ID = 1            # RoBERTa <pad>
Sample = Tuple[str, str, str, int, str]        # the reference's metadata row


# ---------------------------------------------------------------------------------------------------------------------
# data set

def read_annotations(root: str) -> List[Tuple[str, str]]:
    """jhmdb_annotation.txt -> [(video_id, query)] in file order (the first line is the header, as pandas.read_csv takes it)."""
    with open(os.path.join(root, "jhmdb_annotation.txt"), newline="") as f:
        rows = [r for r in csv.reader(f) if r]
    return [(r[0], r[1]) for r in rows[1:]]


def video_folders(root: str) -> Tuple[Dict[str, str], Dict[str, str]]:
    """({video: its frame folder}, {video: its puppet_mask.mat})"""
    frames = {os.path.basename(p): p for p in sorted(glob.glob(os.path.join(root, "Rename_Images", "*", "*")))}
    masks = {os.path.basename(os.path.dirname(p)): p
             for p in sorted(glob.glob(os.path.join(root, "puppet_mask", "*", "*", "puppet_mask.mat")))}
    return frames, masks


def load_part_masks(path: str) -> np.ndarray:
    """puppet_mask.mat -> [frames, H, W] (non-zero = the actor)."""
    import scipy.io
    return scipy.io.loadmat(path)["part_mask"].transpose(2, 0, 1)


def draw_samples(root: str, seed: int = 0) -> List[Sample]:
    """Three frames per (video, query), drawn as the reference draws them (dataset :61-71) from random.Random(seed)."""
    rng = random.Random(seed)
    frame_dirs, mask_files = video_folders(root)
    samples = []
    for video, query in read_annotations(root):
        paths = sorted(glob.glob(os.path.join(frame_dirs[video], "*.png")))
        paths = paths[:len(load_part_masks(mask_files[video]))]          # frames past the last mask cannot be scored
        for p in sorted(rng.sample(paths, FRAMES_PER_QUERY)):
            samples.append((video, p, mask_files[video], len(paths), query))
    return samples


def write_samples(samples: Sequence[Sample], path: str) -> None:
    with open(path, "w") as f:
        json.dump([list(s) for s in samples], f)


def read_samples(path: str) -> List[Sample]:
    with open(path) as f:
        return [(str(v), str(p), str(m), int(n), str(q)) for v, p, m, n, q in json.load(f)]


def frame_number(frame_path: str) -> int:
    return int(os.path.basename(frame_path).split(".")[0])


def window_frames(frame: int, total_frames: int, window: int = WINDOW) -> List[int]:
    """The 1-indexed frames of the window around `frame`: frame - window // 2 .. frame + (window + 1) // 2 - 1, each clamped to
    [1, total_frames] (dataset :98-103).  `frame` sits at position window // 2."""
    return [min(max(i, 1), total_frames) for i in range(frame - window // 2, frame + (window + 1) // 2)]


def valid_indices(clips: int, window: int = WINDOW) -> List[int]:
    """The '(b t)' index of every clip's centre frame (trainer.py:262-270)."""
    return [window // 2 + window * b for b in range(clips)]


def clean_query(query: str) -> str:
    return " ".join(query.lower().split())


def image_id(video: str, frame: int) -> str:
    return f"v_{video}_f_{frame}"


def make_synthetic(root: str, videos: int = 2, frames: int = 12, height: int = 240, width: int = 320, seed: int = 0) -> str:
    """Writes a `videos`-video tree in the JHMDB-Sentences layout: PNG frames, puppet_mask.mat (one drifting ellipse; every
    second video has one mask fewer than frames, as the real set does for some), the CSV."""
    import scipy.io
    from PIL import Image
    from . import synthetic_dataset as SD
    actions = ("walk", "wave", "jump")
    rows = []
    for v in range(videos):
        name, action = f"video{v:03d}", actions[v % len(actions)]
        folder = os.path.join(root, "Rename_Images", action, name)
        os.makedirs(folder, exist_ok=True)
        for t in range(frames):
            Image.fromarray(SD._frame(np.random.default_rng(seed * 1000 + v), height, width, t)).save(
                os.path.join(folder, f"{t + 1:05d}.png"))
        n_masks = frames - (v % 2)
        maps = SD.blob_label_maps(seed * 1000 + v, n_masks, height, width, objects=1)
        mdir = os.path.join(root, "puppet_mask", action, name)
        os.makedirs(mdir, exist_ok=True)
        scipy.io.savemat(os.path.join(mdir, "puppet_mask.mat"), {"part_mask": np.ascontiguousarray(maps.transpose(1, 2, 0))})
        rng = np.random.default_rng(seed * 1000 + 500 + v)
        words = [SD.WORDS[int(i)] for i in rng.integers(0, len(SD.WORDS), int(rng.integers(3, 8)))]
        rows.append((name, "  ".join(words).capitalize()))
    with open(os.path.join(root, "jhmdb_annotation.txt"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("video_id", "query"))
        w.writerows(rows)
    return root


# ---------------------------------------------------------------------------------------------------------------------
# model

def pad_expressions(token_ids: Sequence[torch.Tensor]):
    """[ids [1,L_b]] -> {'input_ids', 'attention_mask'} [B,L]: <pad> and attention 0 behind the shorter ones, what
    tokenizer(..., padding='longest') gives the reference."""
    L = max(int(t.numel()) for t in token_ids)
    ids = torch.full((len(token_ids), L), PAD_ID, dtype=torch.long)
    attn = torch.zeros(len(token_ids), L, dtype=torch.long)
    for b, t in enumerate(token_ids):
        ids[b, :t.numel()] = t.view(-1)
        attn[b, :t.numel()] = 1
    return {"input_ids": ids, "attention_mask": attn}


@torch.no_grad()
def forward_center(model, clips: Sequence[torch.Tensor], token_ids: Sequence[torch.Tensor], window: int = WINDOW):
    """B windows [T,3,h,w] of one geometry (on the device) and their expressions -> the model's outputs for the centre
    frames: pred_masks [1,B,Q,h/4,w/4], pred_cls [1,B,Q,1].  Every sample gets its B = 1 result (the VOC module clusters each
    clip on its own: forward_tail(voc_per_clip=True))."""
    B = len(clips)
    T, _, h, w = clips[0].shape
    device = clips[0].device
    samples = NestedTensor(torch.stack(list(clips), 1), torch.zeros(T, B, h, w, dtype=torch.bool, device=device), unpadded=True)
    text = {k: v.to(device) for k, v in pad_expressions(token_ids).items()}
    idx = torch.tensor([window // 2 + T * b for b in range(B)], device=device)
    state = model.forward_head(samples, idx, text)
    return model.forward_tail(state, [[{"size": (h, w)}] * B], voc_per_clip=B > 1)


class WindowReader:
    """Decoded and pre-processed windows.  The three annotated frames of a (video, query) lie in one short video, so a
    video's frames are decoded once and kept as uint8 while its samples go by."""

    def __init__(self, device, size: int = 320, max_size: Optional[int] = 576):
        self.pre = clip_io.FramePreprocessor(device, size, max_size)
        self._video, self._frames = None, {}

    def window(self, folder: str, frames: Sequence[int]):
        """-> (clip [T,3,h,w] on the device, (H0, W0))"""
        if folder != self._video:
            self._video, self._frames = folder, {}
        for i in set(frames) - set(self._frames):
            self._frames[i] = clip_io.decode_frame(os.path.join(folder, f"{i:05d}.png"))
        stack = torch.from_numpy(np.stack([self._frames[i] for i in frames]))
        return self.pre(stack)


@torch.no_grad()
def run(model, tokenize: Tokenize, root: str, out_dir: str, rank: int = 0, world: int = 1, device="cuda",
        samples_file: Optional[str] = None, seed: int = 0, group: int = 1, save_predictions: bool = False,
        size: int = 320, max_size: Optional[int] = 576) -> Dict:
    """Scores every sample and writes <out>/metrics.json and <out>/ious.csv (and <out>/samples.json when the samples were drawn
    here, <out>/predictions.json with save_predictions).  group: consecutive samples of one geometry share a forward and the
    K6c launch behind it.  Returns the statistics; stats['metrics'] is the reference's eval_metrics dict."""
    if world != 1:
        raise ValueError("the metrics cover every sample of the set, so the JHMDB-Sentences driver runs in one process (world = 1)")
    if int(group) != group or group < 1:
        raise ValueError("group must be a positive sample count")
    os.makedirs(out_dir, exist_ok=True)
    if samples_file:
        samples = read_samples(samples_file)
    else:
        samples = draw_samples(root, seed)
        write_samples(samples, os.path.join(out_dir, "samples.json"))
    frame_dirs, mask_files = video_folders(root)
    device = torch.device(device)
    reader = WindowReader(device, size, max_size)
    Q = model.num_queries
    stats = {"samples": len(samples), "expressions": len(samples), "batches": 0, "seconds_input": 0.0}
    scored = []                 # (ids of the batch, scores [B,Q] and counts [B,Q,3] on the device): nothing is waited for
    predictions = []
    masks_of, masks_path = None, None
    t0 = time.perf_counter()

    def flush(batch):
        if not batch:
            return
        clips = [b["clip"] for b in batch]
        out = forward_center(model, clips, [b["ids"] for b in batch])
        logits = out["pred_masks"][0]                                       # [B,Q,hm,wm]
        scores = out["pred_cls"][0, :, :, 0].sigmoid()
        padded = tuple(clips[0].shape[-2:])
        resized = [padded] * len(batch)                                     # one geometry per batch: nothing is padded
        original = [b["orig"] for b in batch]
        gt_bits, gt_off = center_frame.pack_ground_truth([b["gt"] for b in batch], device)
        bits, counts = center_frame.center_frame_bits(logits, padded, resized, original, gt_bits, gt_off,
                                                      masks=save_predictions)
        scored.append(([b["image_id"] for b in batch], scores, counts))
        stats["batches"] += 1
        if save_predictions:
            host, host_scores = bits.cpu(), scores.cpu()
            for n, b in enumerate(batch):
                planes = center_frame.sample_masks(host, original, Q, n).numpy()
                for q in range(Q):
                    predictions.append({"image_id": b["image_id"], "category_id": 1, "score": host_scores[n, q].item(),
                                        "segmentation": {"size": [int(v) for v in b["orig"]],
                                                         "counts": center_frame.rle_counts(planes[q], b["orig"])}})

    batch = []
    for video, frame_path, _, total_frames, query in samples:
        t1 = time.perf_counter()
        frame = frame_number(frame_path)
        if mask_files[video] != masks_path:
            masks_path, masks_of = mask_files[video], load_part_masks(mask_files[video])
        clip, orig = reader.window(frame_dirs[video], window_frames(frame, total_frames))
        gt = masks_of[frame - 1]
        if tuple(gt.shape) != tuple(orig):
            raise ValueError(f"{video}: the masks are {tuple(gt.shape)}, the frames {tuple(orig)}")
        stats["seconds_input"] += time.perf_counter() - t1
        item = {"clip": clip, "orig": (int(orig[0]), int(orig[1])), "gt": gt, "ids": tokenize(clean_query(query)),
                "image_id": image_id(video, frame)}
        if batch and (len(batch) == group or batch[0]["clip"].shape != clip.shape):
            flush(batch)
            batch = []
        batch.append(item)
    flush(batch)

    ids, best_counts, best_q = [], [], []
    for batch_ids, scores, counts in scored:                                # the first host read of any result
        best = center_eval.select_best(scores.cpu().numpy())
        c = counts.cpu().numpy()
        ids += batch_ids
        best_q += best.tolist()
        best_counts += [c[n, q].tolist() for n, q in enumerate(best)]
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    stats["seconds"] = time.perf_counter() - t0
    m = center_eval.metrics(best_counts)
    stats["metrics"] = center_eval.eval_metrics(m)
    print(stats["metrics"])
    with open(os.path.join(out_dir, "metrics.json"), "w") as f:
        json.dump({**stats["metrics"], "num_samples": m["num_samples"]}, f, indent=1)
    with open(os.path.join(out_dir, "ious.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("image_id", "query", "iou", "inter", "pred_area", "gt_area"))
        for i, q, iou, c in zip(ids, best_q, m["ious"], best_counts):
            w.writerow((i, q, repr(iou), *c))
    if save_predictions:
        with open(os.path.join(out_dir, "predictions.json"), "w") as f:
            json.dump(predictions, f)
    return stats
