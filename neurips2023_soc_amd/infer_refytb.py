"""Ref-YouTube-VOS inference driver: the per-process body of the reference's infer_refytb.py
(`sub_processor`, :112-285) on the MI355X pipeline.

    for each video (this rank's share)            reference :160, split :84-109
      for each expression of the video            :181
        frames -> resized, normalised clip        :191-207   here: decoded once per VIDEO, K9 on the GPU
        forward, pick the best query              :209-226   SOC.forward (K1-K5, K7, K8) + select_trajectory
        up-sample to the original size, > 0.5     :230-231   K6
        write <out>/<video>/<exp_id>/<frame>.png  :269-277   8-bit 'L' PNG, 0 / 255, from a writer pool

Dataset layout (reference :62-82): <root>/valid/JPEGImages/<video>/<frame>.jpg and
<root>/meta_expressions/valid/meta_expressions.json = {"videos": {video: {"frames": [...],
"expressions": {exp_id: {"exp": str}}}}}.  Visualisation (:233-266) is not part of the hot path.
"""
from __future__ import annotations

import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch

from . import clip_io
from .infer import ClipInferencer

Tokenize = Callable[[str], torch.Tensor]


def split_videos(videos: Sequence[str], rank: int, world: int):
    """Contiguous shares, the remainder to the last rank (reference infer_refytb.py:92-99)."""
    per = len(videos) // world
    return list(videos[rank * per:] if rank == world - 1 else videos[rank * per:(rank + 1) * per])


def save_binary_mask(mask: np.ndarray, path: str) -> None:
    """bool/0-1 [H,W] -> 8-bit 'L' PNG with 0 / 255 (reference :272-277).  Same mode and pixels as the reference writes.
    Written by the run-length encoder of libsoc_host.so (png_fast.py: ~0.2 ms of CPU per 720p mask where zlib needs 1.9 at its
    fastest level and 3.0 at Pillow's default -- at 8 masks per clip the PNG encoder was the larger half of the host's work,
    profiles/r04_files_to_png.json); SOC_PNG=pillow writes through Pillow instead (SOC_PNG_LEVEL, default Pillow's own)."""
    from . import png_fast
    if png_fast.use_pillow():
        from PIL import Image
        Image.fromarray(mask.astype(np.uint8) * 255, mode="L").save(path, **png_fast.pillow_save_kwargs())
    else:
        png_fast.save(path, mask, binarize=True)


def save_packed_mask(bits: np.ndarray, width: int, path: str) -> None:
    """save_binary_mask for a bit-packed mask [H, RB] of `width` pixels (packed_masks.py): the same file, byte for byte,
    encoded straight from the bits (png_fast.encode_bits); with the Pillow writer the mask is unpacked first."""
    from . import png_fast
    if png_fast.use_pillow():
        from . import packed_masks
        save_binary_mask(packed_masks.unpack(bits, width), path)
    else:
        png_fast.save_bits(path, bits, width)


def load_meta(root: str, split: str = "valid"):
    img_folder = os.path.join(root, split, "JPEGImages")
    with open(os.path.join(root, "meta_expressions", split, "meta_expressions.json")) as f:
        return img_folder, json.load(f)["videos"]


class _Scorer:
    """Per-expression J&F (refytb_eval, K27b) of the masks against a ground-truth tree, while they are still on the device.  A
    video's label maps are decoded once, on a reader thread from the moment the driver reaches the video, uploaded when its
    first expression arrives and dropped after its last.  Nothing is waited for here: the counts stay on the device until
    finish()."""

    def __init__(self, eval_root: str, split: str, videos: Sequence[str], device):
        from . import refytb_eval
        self.re, self.split, self.device = refytb_eval, split, device
        self.dataset = refytb_eval.RefYtbDataset(eval_root, split, videos)
        self.obj_of = {v: dict(self.dataset.expressions(v)) for v in self.dataset.videos}     # a missing obj_id raises here
        self.gt = {}                # video -> [labels on the device, expressions still to come]
        self.expected = {}          # video -> expressions the driver will send
        self.reader = ThreadPoolExecutor(max_workers=2)
        self.reading = {}           # video -> future of its label maps (PNG decoding beside the forwards)
        self.scored = []            # (video, exp_ids, obj_ids, counts [E,T,6] on the device), in arrival order

    def begin(self, video: str, expressions: int) -> None:
        self.expected[video] = expressions
        if expressions and video not in self.reading and video not in self.gt:
            self.reading[video] = self.reader.submit(self.dataset.masks, video)

    @staticmethod
    def in_place(bits: Sequence[torch.Tensor]):
        """Packed masks of several expressions -> (pred_bits, exp_stride) for jf_bits.jf_counts_bits: the first one's view and
        the distance in bytes when they lie evenly spaced in one buffer (the slices of a group's K6b output), a stacked copy
        otherwise."""
        first = bits[0]
        if len(bits) == 1:
            return (first, None) if first.is_contiguous() and first.data_ptr() % 8 == 0 else (first.contiguous().clone()[None], None)
        step = bits[1].data_ptr() - first.data_ptr()
        even = all(b.is_contiguous() and b.shape == first.shape and b.data_ptr() == first.data_ptr() + k * step
                   and b.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() for k, b in enumerate(bits))
        if even and step >= first.numel() and step % 8 == 0 and first.data_ptr() % 8 == 0:
            return first, step
        return torch.stack(list(bits)), None

    def score(self, video: str, exp_ids: Sequence[str], bits: Sequence[torch.Tensor], width: int) -> None:
        """bits: one packed uint8 [T,H0,RB] mask tensor per expression of `video`, all scored in ONE call."""
        if video not in self.gt:
            maps = self.reading.pop(video).result()
            self.gt[video] = [torch.from_numpy(maps).to(self.device), self.expected[video]]
        entry = self.gt[video]
        gt = entry[0]
        want = (gt.shape[0], gt.shape[1], 8 * (-(-gt.shape[2] // 64)))
        if tuple(bits[0].shape) != want or int(width) != gt.shape[2]:
            raise ValueError(f"{video}: ground truth {tuple(gt.shape)} does not match the output "
                             f"({bits[0].shape[0]}, {bits[0].shape[1]}, {int(width)}) (frames, height, width)")
        for exp_id in exp_ids:
            if exp_id not in self.obj_of[video]:
                raise KeyError(f"{self.dataset.meta_path}: videos['{video}']['expressions'] has no '{exp_id}'")
        obj_ids = [self.obj_of[video][e] for e in exp_ids]
        pred, stride = self.in_place(bits)
        self.scored.append((video, list(exp_ids), obj_ids, self.re.video_counts(gt, obj_ids, pred, exp_stride=stride)))
        entry[1] -= len(exp_ids)
        if entry[1] <= 0:
            del self.gt[video]

    def finish(self, out_dir: str) -> Dict:
        self.reader.shutdown()
        result = self.re.RefYtbJF()
        for video, exp_ids, obj_ids, counts in self.scored:
            result.add_counts(video, exp_ids, obj_ids, counts.cpu().numpy())
        os.makedirs(out_dir, exist_ok=True)
        self.re.write_csvs(result, out_dir, self.split)
        return {"measures": list(self.re.G_MEASURES), "global": result.global_row(),
                "per_expression": [list(r) for r in result.per_expression()]}


PREFETCH_VIDEOS = 4          # videos decoded ahead of the one on the GPU (a 720p clip of 8 frames is 22 MB of pinned staging)


@torch.no_grad()
def run(model, tokenize: Tokenize, root: str, out_dir: str, rank: int = 0, world: int = 1, device="cuda",
        split: str = "valid", size: int = 360, max_size: Optional[int] = 640, use_graphs: bool = False,
        decode_workers: int = 8, writer_workers: int = 16, videos: Optional[Sequence[str]] = None,
        engine: Optional[ClipInferencer] = None, pad_tokens_to: Optional[int] = 32, group: int = 1,
        packed_masks: bool = False, eval_root: Optional[str] = None, share_video: bool = False) -> Dict:
    """Process this rank's videos; returns counters + timings.  share_video: all expressions of a video go to the engine in ONE
    call (ClipInferencer(share_video=True): submit_expressions with graphs, run_expressions without), which runs the video side
    of the forward once for them; files, tags, scoring and packed masks are as without it.  eval_root: a tree with <split>/Annotations and a
    meta_expressions.json whose expressions carry obj_id.  When given, every expression's masks are scored against the object it
    names while they are on the device (refytb_eval, K27b: the bits K6b wrote are read in place, the expressions of one video
    that arrive in one group in one call; byte masks are packed on the device first): stats["jf"] holds the global row and the
    per-expression rows, and the two CSVs are written into out_dir.  The PNGs and everything else the driver does are the same
    with and without it.  packed_masks: the masks leave the GPU one bit per pixel (K6b, once
    per group of one original size), the pinned buffers and the host copy are [T,H0,RB] uint8 -- an eighth -- and the writers encode
    the PNGs from the bits; the files are the same.  group > 1 (with use_graphs): consecutive clips of one
    geometry share every launch of the forward, each still getting its single-clip result (ClipInferencer(group=...)).  `tokenize(expression) -> int64 [1,L]`
    (RobertaTokenizerFast in production; no vocabulary files exist offline, so the caller supplies it)."""
    img_folder, data = load_meta(root, split)
    todo = split_videos(sorted(data.keys()) if videos is None else list(videos), rank, world)
    scorer = None
    if eval_root is not None:
        if world != 1:
            raise ValueError("eval_root: the tables cover every video of the set, so scoring runs in one process (world = 1)")
        scorer = _Scorer(eval_root, split, todo, device)
    engine = engine or ClipInferencer(model, device, use_graphs=use_graphs, pad_tokens_to=pad_tokens_to, group=group,
                                      packed_masks=packed_masks, share_video=share_video)
    if share_video and not getattr(engine, "share_video", False):
        raise ValueError("share_video of run() needs an engine built with share_video=True")
    if bool(getattr(engine, "packed_masks", False)) != bool(packed_masks):
        raise ValueError("packed_masks of run() and of the engine it was given disagree")
    cache = clip_io.VideoClipCache(clip_io.FramePreprocessor(device, size, max_size), workers=decode_workers)
    stats = {"videos": 0, "expressions": 0, "frames": 0, "seconds_input": 0.0, "seconds_model": 0.0}
    pending = []
    t0 = time.perf_counter()

    def flush(job):
        """clip i's masks -> PNG jobs; called after clip i+1 has been enqueued, so the D2H copy, the numpy
        view and the job submission overlap the next forward instead of idling the GPU"""
        host, done, save_dir, names, width = job
        done.synchronize()
        masks = host.numpy().copy()            # the pinned buffer is reused two clips later (packed: an eighth of the bytes)
        for j, name in enumerate(names):
            path = os.path.join(save_dir, name + ".png")
            if width is None:
                pending.append(writers.submit(save_binary_mask, masks[j], path))
            else:
                pending.append(writers.submit(save_packed_mask, masks[j], width, path))

    pinned: Dict = {}                      # two host buffers per mask shape, reused (pinning is slow)

    def host_buffer(shape, slot, dtype):
        key = (tuple(shape), slot, dtype)
        if key not in pinned:
            pinned[key] = torch.empty(tuple(shape), dtype=dtype, pin_memory=True)
        return pinned[key]

    d2h = torch.cuda.Stream(device=device)    # mask download overlaps the next clip's forward

    streaming = engine.use_graphs        # graphs: software-pipelined replays, results arrive one replay late
    # downloads left in flight behind the newest results: with a group pipeline (engine.group clips per replay) the results
    # of a group arrive together, right behind the replay of the NEXT group -- waiting for them at once would hold the host
    # for that whole replay
    lag = engine.group if streaming else 1

    def enqueue_download(res):
        """masks of a finished clip -> pinned host buffer on the d2h stream; returns the job for flush()"""
        save_dir, names = res["tag"][:2]
        masks, width = (res["masks_packed"], res["mask_size"][1]) if packed_masks else (res["masks"], None)
        host = host_buffer(masks.shape, enqueue_download.n % (2 * lag + 2), masks.dtype)
        enqueue_download.n += 1
        d2h.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(d2h):
            host.copy_(masks, non_blocking=True)
            masks.record_stream(d2h)
            done = torch.cuda.Event()
            done.record()
        return (host, done, save_dir, names, width)
    enqueue_download.n = 0

    import collections
    jobs = collections.deque()           # downloads in flight, oldest first

    def score(results):
        """the results of one replay (or one eager call), video by video: each video's expressions in one call"""
        t3 = time.perf_counter()
        i = 0
        while i < len(results):
            video = results[i]["tag"][2]
            j = i
            while j < len(results) and results[j]["tag"][2] == video:
                j += 1
            run = results[i:j]
            if packed_masks:
                bits, width = [r["masks_packed"] for r in run], run[0]["mask_size"][1]
            else:
                from . import packed_masks as PM
                bits, width = [PM.pack(r["masks"]) for r in run], run[0]["masks"].shape[-1]
            scorer.score(video, [r["tag"][3] for r in run], bits, width)
            i = j
        stats["seconds_eval"] = stats.get("seconds_eval", 0.0) + time.perf_counter() - t3

    def handle(results):
        for res in results:
            jobs.append(enqueue_download(res))
            while len(jobs) > lag:
                flush(jobs.popleft())
        if scorer is not None and results:
            score(results)

    with ThreadPoolExecutor(max_workers=writer_workers) as writers:
        for vi, video in enumerate(todo):
            frames = data[video]["frames"]
            paths = clip_io.frame_paths(img_folder, video, frames)
            # decode the NEXT videos' JPEGs while this one is on the GPU.  Several ahead (round 6): with launch groups a submit returns
            # at once and the host thread sits in the next replay for a whole group's GPU time -- a video with one expression is
            # 5 ms of GPU against ~8 ms of decode, and with one video of lookahead the decoder idled during every replay
            for ahead in range(1, PREFETCH_VIDEOS + 1):
                if vi + ahead < len(todo):
                    nxt = todo[vi + ahead]
                    cache.prefetch(clip_io.frame_paths(img_folder, nxt, data[nxt]["frames"]))
            if scorer is not None:
                scorer.begin(video, len(data[video]["expressions"]))
            expressions = data[video]["expressions"]
            if share_video and expressions:
                t1 = time.perf_counter()
                clip, orig = cache.get(paths)
                ids = [tokenize(item["exp"]).pin_memory().to(device, non_blocking=True) for item in expressions.values()]
                t2 = time.perf_counter()
                tags = [(os.path.join(out_dir, video, exp_id), frames, video, exp_id) for exp_id in expressions]
                for tag in tags:
                    os.makedirs(tag[0], exist_ok=True)
                if streaming:
                    handle(engine.submit_expressions(clip, ids, tags, orig))   # results of the PREVIOUS replay, if any
                else:
                    results = engine.run_expressions(clip, ids, orig)
                    for res, tag in zip(results, tags):
                        res["tag"] = tag
                    handle(results)
                stats["seconds_input"] += t2 - t1
                stats["seconds_model"] += time.perf_counter() - t2
                stats["expressions"] += len(ids)
                stats["frames"] += len(frames) * len(ids)
                expressions = {}
            for exp_id, item in expressions.items():
                t1 = time.perf_counter()
                clip, orig = cache.get(paths)                                  # decoded / resized once per video
                ids = tokenize(item["exp"]).pin_memory().to(device, non_blocking=True)
                t2 = time.perf_counter()
                save_dir = os.path.join(out_dir, video, exp_id)
                os.makedirs(save_dir, exist_ok=True)
                if streaming:
                    handle(engine.submit(clip, ids, (save_dir, frames, video, exp_id), orig))  # results of the PREVIOUS replay, if any
                else:
                    res = engine(clip, ids, orig)                              # [T,H0,W0] bool, still in flight
                    res["tag"] = (save_dir, frames, video, exp_id)
                    handle([res])
                stats["seconds_input"] += t2 - t1
                stats["seconds_model"] += time.perf_counter() - t2
                stats["expressions"] += 1
                stats["frames"] += len(frames)
            stats["videos"] += 1
        if streaming:
            handle(engine.drain())
        while jobs:
            flush(jobs.popleft())
        t_tail = time.perf_counter()
        for f in pending:
            f.result()
        stats["seconds_writer_tail"] = time.perf_counter() - t_tail
    torch.cuda.synchronize()
    cache.close()
    stats.update(seconds=time.perf_counter() - t0, cache_hits=cache.hits, cache_misses=cache.misses)
    stats.update({k: v for k, v in getattr(engine, "stats", {}).items()})       # group replays, part-filled ones, remainders
    if scorer is not None:
        stats["jf"] = scorer.finish(out_dir)
    return stats
