"""Clip-level inference driver: the body of the reference's per-(video, expression) loop
(infer_refytb.py:185-231 without the disk I/O) on top of ClipGraph, plus the clip-parallel
multi-GPU form of its `sub_processor` fan-out (infer_refytb.py:84-109).

    python -m neurips2023_soc_amd.infer --clips 16            # synthetic Ref-YouTube-VOS-like stream
    python -m neurips2023_soc_amd.infer --clips 64 --gpus 8   # starts its 8 ranks itself (reference: -ng 8)
    python -m torch.distributed.run --nproc-per-node 8 -m neurips2023_soc_amd.infer --clips 64 --gpus 8
    python -m neurips2023_soc_amd.infer --dataset refytb --root DATA --out RUNS [--tokenizer DIR] [--checkpoint CKPT]
    python -m neurips2023_soc_amd.infer --dataset davis --root DATA --out RUNS --make-synthetic 4   # writes DATA first
    python -m neurips2023_soc_amd.infer --dataset refytb --root DATA --out RUNS --packed-masks --eval-refytb GT   # scores RUNS
    python -m neurips2023_soc_amd.infer --dataset jhmdb --root DATA --out RUNS [--samples FILE] [--save-predictions]   # P@K, IoU
"""
from __future__ import annotations

import argparse
import json
import os
import time
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import clip_parallel as CP
from . import postprocessing as P
from .graph_runner import ClipGraph, PipelinedClipGraph, group_pipeline_class, pipeline_class, shared_group_pipeline_class
from .nested_tensor import NestedTensor


class _WeightsEpoch:
    """load_state_dict post-hook on every module of a model: counts the loads (of the model or of any part of it).  A class, not
    a closure, so that a model carrying it can still be pickled and deep-copied."""

    def __init__(self):
        self.n = 0

    def __call__(self, module, incompatible_keys):
        self.n += 1


def weights_epoch(model) -> _WeightsEpoch:
    """The model's load counter (installed on first use).  Captured graphs have the weights' packed images and, for biases and
    norm parameters, the parameters' own addresses baked in: after a load a graph captured before it would compute with a mix
    of old and new weights, so ClipInferencer compares `.n` (one integer, no walk over the parameters) on every call and drops
    its graphs when it moved."""
    epoch = model.__dict__.get("_soc_weights_epoch")
    if epoch is None:
        epoch = model.__dict__["_soc_weights_epoch"] = _WeightsEpoch()
        for m in model.modules():
            m.register_load_state_dict_post_hook(epoch)
    return epoch


class ClipInferencer:
    """model + (optionally) one hipGraph per (T, H, W, L) geometry.  `__call__` returns the reference
    driver's per-clip products: selected query index, its mask logits, and the thresholded full-size
    masks.  use_graphs=True pays off on streams of one geometry (bench, DAVIS 36-frame clips); whole-video
    clips with free-form expressions (Ref-YouTube-VOS: T and L change per call) run eagerly.

    Weights: a `load_state_dict` on the model (or a part of it) and a move of the model to another device and back are noticed
    on the next call, which drops every captured graph and captures afresh under the new weights (weights_epoch; with clips
    still staged or in flight the call raises instead: drain() first).  An in-place edit of single parameters
    (`p.copy_(w)` under no_grad) is seen by the eager forward but NOT by a captured graph: call reset() after it."""

    PAD_ID = 1            # RoBERTa <pad>

    def __init__(self, model, device="cuda", use_graphs: bool = True, max_graphs: int = 4,
                 pad_tokens_to: Optional[int] = None, group: int = 1, packed_masks: bool = False, share_video: bool = False):
        """packed_masks: results carry 'masks_packed' (uint8 [T,H0,RB], one bit per pixel: packed_masks.py) and 'mask_size'
        (H0, W0) instead of 'masks'; a group whose clips share one original size is up-sampled in ONE launch from the record.
        pad_tokens_to: with graphs, pad every expression to this many tokens (<pad> + attention mask 0), so
        that the graph geometry does not depend on the expression.  The reference's outputs are exactly
        invariant to such padding (checked on the reference itself; tests/test_host_plumbing.py checks the
        oracle), which is what tokenizer(..., padding="longest") does to the shorter expressions of a batch."""
        self.model, self.device = model, torch.device(device)
        self.use_graphs, self.max_graphs, self.pad_tokens_to = use_graphs, max_graphs, pad_tokens_to
        # group > 1: the streaming form shares every launch between `group` consecutive clips of one geometry -- of one video or of
        # several (graph_runner.group_pipeline_class: each clip still gets its single-clip result).  A part-filled group --
        # geometry change, end of the stream -- costs a whole replay whatever it holds, so (round 6) a remainder of FEWER than
        # half a group leaves through the one-clip pipeline of the same geometry instead (captured beside the group graph the
        # first time it is needed); half a group or more runs with stale partner slots whose records are dropped.
        if int(group) != group or group < 1:
            raise ValueError("group must be a positive clip count")
        self.group = group
        self.packed_masks = bool(packed_masks)
        # share_video: submit_expressions / run_expressions take ONE clip and all its expressions and run the video side of the
        # forward once for them (SOC.forward_expressions, graph_runner.shared_group_pipeline_class: `group` expression slots per
        # replay).  Off, nothing of it is ever constructed.
        self.share_video = bool(share_video)
        self._shared: Dict[Tuple[int, int, int, int], PipelinedClipGraph] = {}      # shared-video pipelines, in _pipes' budget
        self._shared_active = None   # (key, pipe, [(tag, original_size)] of the expressions in flight)
        self._filling = []           # (tag, original_size) of the clips staged into the group that has not been replayed yet
        self._graphs: Dict[Tuple[int, int, int, int], ClipGraph] = {}
        self._pipes: Dict[Tuple[int, int, int, int], PipelinedClipGraph] = {}
        self._singles: Dict[Tuple[int, int, int, int], PipelinedClipGraph] = {}     # one-clip pipelines for the remainders of groups
        self._active = None          # (key, pipe, tag of the clip in flight)
        self.stats = {"group_replays": 0, "part_filled_replays": 0, "stale_slots": 0, "remainder_singles": 0,
                      "weight_reloads_seen": 0, "shared_video_passes": 0, "shared_expressions": 0}
        watched = use_graphs and isinstance(model, torch.nn.Module)      # (anything else has no load_state_dict to watch)
        self._epoch = weights_epoch(model) if watched else None
        self._probe = next(model.parameters(), None) if watched else None        # re-pointed by model.cpu() / .cuda() / .to()
        self._captured_under = self._weights_state()

    def _weights_state(self):
        if self._epoch is None:
            return None
        return (self._epoch.n, None if self._probe is None else self._probe.data_ptr())

    def _check_weights(self):
        """Drop every graph that was captured under other weights than the model has now.  Two integers per call; not on the
        replay path of a runner (graph_runner), which callers that own their runner drive directly."""
        if self._epoch is not None and self._weights_state() != self._captured_under:
            if self._active is not None or self._filling or self._shared_active is not None:
                raise RuntimeError("the model's weights changed while clips are staged or in flight: drain() before loading weights")
            self.stats["weight_reloads_seen"] += 1
            self.reset()

    def reset(self):
        """Drop every captured graph (and with it the packed weight images and geometry constants it held); the next call of a
        geometry captures again.  Needed by hand after in-place edits of single parameters (`p.copy_`) only."""
        if self._active is not None or self._filling or self._shared_active is not None:
            raise RuntimeError("clips are staged or in flight: drain() first")
        if self._graphs or self._pipes or self._singles or self._shared:
            torch.cuda.synchronize(self.device)              # never drop a graph that may still be replaying
        self._graphs.clear()
        self._pipes.clear()
        self._singles.clear()
        self._shared.clear()
        self._captured_under = self._weights_state()

    def _runner(self, held: Dict, key, runner_class):
        """held[key], built as runner_class()(model, *key, device) on first use, behind the eviction of the oldest runners of `held`."""
        if key not in held:
            while len(held) >= self.max_graphs:              # a graph pins its activation pool: keep few
                torch.cuda.synchronize(self.device)          # never drop a graph that may still be replaying
                held.pop(next(iter(held)))
            held[key] = runner_class()(self.model, *key, self.device)
        return held[key]

    def graph_for(self, T: int, H: int, W: int, L: int) -> ClipGraph:
        return self._runner(self._graphs, (T, H, W, L), lambda: ClipGraph)

    # -- streaming form: the software-pipelined graph (tail of clip i beside the head of clip i+1) ---------------
    def _pad_tokens(self, token_ids: torch.Tensor):
        ids, attn = token_ids.view(1, -1), None
        L = ids.shape[-1]
        if self.pad_tokens_to is not None and L < self.pad_tokens_to:
            extra = self.pad_tokens_to - L
            attn = torch.cat([torch.ones_like(ids), ids.new_zeros(1, extra)], 1)
            ids = torch.cat([ids, ids.new_full((1, extra), self.PAD_ID)], 1)
        return ids, attn

    def _masks_into(self, res: Dict, masks: torch.Tensor, original_size, packed: Optional[torch.Tensor] = None):
        """The full-size masks of one clip, in the form this engine was built for; `packed`: already up-sampled with its group."""
        if not self.packed_masks:
            res["masks"] = P.upsample_and_threshold(masks, original_size)
        else:
            res["masks_packed"] = P.upsample_and_threshold_packed(masks, original_size) if packed is None else packed
            res["mask_size"] = (int(original_size[0]), int(original_size[1]))

    def _unpack(self, rec: torch.Tensor, key, tag, original_size, packed: Optional[torch.Tensor] = None):
        T, H, W, _ = key
        Q = self.model.num_queries
        hm, wm = -(-H // 4), -(-W // 4)
        masks = rec[1 + T * Q:].view(T, hm, wm)
        res = {"tag": tag, "query": rec[0].to(torch.int64), "mask_logits": masks, "pred_cls": rec[1:1 + T * Q].view(T, Q)}
        if original_size is not None:
            self._masks_into(res, masks, original_size, packed)
        return res

    def _pipeline(self, key):
        while self._shared and key not in self._pipes and len(self._shared) + len(self._pipes) >= self.max_graphs:
            torch.cuda.synchronize(self.device)              # shared-video pipelines (drained by now) sit in the same budget
            self._shared.pop(next(iter(self._shared)))
        return self._runner(self._pipes, key, lambda: pipeline_class() if self.group == 1 else group_pipeline_class(self.group))

    def _single_pipeline(self, key):
        return self._runner(self._singles, key, pipeline_class)

    def _unpack_rows(self, rec: torch.Tensor, key, clips):
        """rec: what a replay or a flush of this engine's pipeline hands out -- one record for group = 1, a row per slot
        otherwise; clips: the (tag, original_size) of the slots that were filled."""
        rows = rec if self.group > 1 else [rec]
        packed = None
        sizes = {None if osz is None else (int(osz[0]), int(osz[1])) for _, osz in clips}
        if self.packed_masks and self.group > 1 and len(clips) > 1 and len(sizes) == 1 and None not in sizes \
                and rec.dim() == 2 and rec.stride(1) == 1:
            # one original size in the group: K6b reads every filled row's mask logits where the record holds them
            from . import packed_masks as PM
            T, H, W, _ = key
            first = rec[0, 1 + T * self.model.num_queries:].view(T, -(-H // 4), -(-W // 4))
            packed = PM.upsample_threshold_bits(first, sizes.pop(), clip_stride=rec.stride(0), clips=len(clips))
        if packed is None:
            return [self._unpack(rows[b], key, tag, osz) for b, (tag, osz) in enumerate(clips)]
        return [self._unpack(rows[b], key, tag, osz, packed=packed[b]) for b, (tag, osz) in enumerate(clips)]

    def _replay(self):
        """Replay the group that has been staged; -> result dicts of the group replayed one call earlier."""
        key, pipe, in_flight = self._active
        rec = pipe.replay()
        filled, self._filling = self._filling, []
        if self.group > 1:
            self.stats["group_replays"] += 1
            if len(filled) < self.group:
                self.stats["part_filled_replays"] += 1
                self.stats["stale_slots"] += self.group - len(filled)
        self._active = (key, pipe, filled)
        if rec is None or not in_flight:
            return []
        return self._unpack_rows(rec, key, in_flight)

    @torch.no_grad()
    def submit(self, clip: torch.Tensor, token_ids: torch.Tensor, tag, original_size=None):
        """Streaming form of __call__ for use_graphs=True: submits `clip` and returns the LIST of result dicts that became
        available -- those of the group of clips replayed one replay earlier (group = 1: the clip submitted before this one),
        preceded by whatever a geometry change had to drain; often empty.  Every result carries the `tag` / `original_size`
        given at its own submit.  Results: 'tag', 'query', 'mask_logits' (a view of the graph's record: consume it, e.g.
        through 'masks', before the next submit), 'pred_cls', 'masks' when original_size was given ('masks_packed' and
        'mask_size' instead with packed_masks=True).  `clip` may be reused by
        the caller as soon as submit returns (it has been copied into the graph's static input)."""
        if not self.use_graphs:
            raise RuntimeError("submit() streams through hipGraphs; construct with use_graphs=True")
        self._check_weights()
        T, _, H, W = clip.shape
        ids, attn = self._pad_tokens(token_ids)
        key = (T, H, W, ids.shape[-1])
        out = []
        if self._shared_active is not None:
            out += self._drain_shared()                           # expressions of a shared-video call are still in flight
        if self._active is not None and self._active[0] != key:
            out += self.drain()                                   # geometry change: finish what is staged and in flight
        pipe = self._pipeline(key)
        if self._active is None:
            self._active = (key, pipe, [])
        pipe.stage_inputs(clip, ids, attn, slot=len(self._filling))
        self._filling.append((tag, original_size))
        if len(self._filling) == self.group:
            out += self._replay()
        return out

    def _remainder_through_singles(self):
        """A part-filled group of fewer than group / 2 clips: the group in flight is flushed, then the staged clips -- read back from
        the group graph's static input slots, the caller may have reused its tensors -- go one by one through the one-clip
        pipeline of the geometry.  r clips cost r one-clip replays (6.2 ms each at the BASELINE geometry) instead of a whole
        group replay (49 ms for ten)."""
        key, pipe, in_flight = self._active
        out = []
        for rec in pipe.flush():
            out += self._unpack_rows(rec, key, in_flight)
        staged, self._filling = self._filling, []
        single = self._single_pipeline(key)
        for b, (tag, osz) in enumerate(staged):
            single.stage_inputs(pipe.clip[:, b].contiguous(), pipe.ids[b], pipe.attn[b])
            rec = single.replay()
            if rec is not None:                                   # the record of the clip staged one replay earlier
                out.append(self._unpack(rec.clone(), key, *staged[b - 1]))
        for rec in single.flush():
            out.append(self._unpack(rec, key, *staged[-1]))
        self.stats["remainder_singles"] += len(staged)
        self._active = None
        return out

    @torch.no_grad()
    def drain(self):
        """Finish what is staged and in flight: list of result dicts.  A part-filled group runs with stale partner slots when it
        is at least half full, through the one-clip pipeline otherwise (_remainder_through_singles)."""
        if self._shared_active is not None:
            return self._drain_shared()
        if self._active is None:
            return []
        out = []
        if self._filling:
            if self.group > 1 and 2 * len(self._filling) < self.group:
                return self._remainder_through_singles()
            out += self._replay()
        key, pipe, in_flight = self._active
        self._active = None
        for rec in pipe.flush():
            out += self._unpack_rows(rec, key, in_flight)
        return out

    # -- shared-video form: one clip, all its expressions, one pass over the video side per replay ----------------
    def _shared_pipeline(self, key):
        """The shared-video pipeline of a geometry; it and the pipelines of _pipes share one budget of max_graphs."""
        if key not in self._shared:
            while len(self._shared) + len(self._pipes) >= self.max_graphs:
                torch.cuda.synchronize(self.device)          # never drop a graph that may still be replaying
                held = self._pipes if self._pipes else self._shared
                held.pop(next(iter(held)))
            self._shared[key] = shared_group_pipeline_class(self.group)(self.model, *key, self.device)
        return self._shared[key]

    def _pad_expressions(self, token_ids, at_least: Optional[int]):
        """[ids [1,L_e]] -> ([ids [1,L]], [attn [1,L] or None]) with L = the longest expression (`at_least`, if longer):
        <pad> + attention mask 0 behind the shorter ones, what tokenizer(..., padding="longest") does."""
        L = max(int(t.numel()) for t in token_ids)
        if at_least is not None:
            L = max(L, at_least)
        ids, attns = [], []
        for t in token_ids:
            t = t.view(1, -1)
            extra = L - t.shape[-1]
            if extra:
                attns.append(torch.cat([torch.ones_like(t), t.new_zeros(1, extra)], 1))
                t = torch.cat([t, t.new_full((1, extra), self.PAD_ID)], 1)
            else:
                attns.append(None)
            ids.append(t)
        return ids, attns

    def _unpack_shared(self, rec: torch.Tensor, key, filled):
        """rec [group, R] of a shared-video replay; filled: (tag, original_size) of its filled slots (one clip: one size).  The
        rows behind them are stale slots and are never handed out."""
        packed = None
        osz = filled[0][1]
        if self.packed_masks and osz is not None and len(filled) > 1 and rec.stride(1) == 1:
            from . import packed_masks as PM            # K6b over the filled rows, read where the record holds them
            T, H, W, _ = key
            first = rec[0, 1 + T * self.model.num_queries:].view(T, -(-H // 4), -(-W // 4))
            packed = PM.upsample_threshold_bits(first, (int(osz[0]), int(osz[1])), clip_stride=rec.stride(0), clips=len(filled))
        return [self._unpack(rec[s], key, tag, size, packed=None if packed is None else packed[s])
                for s, (tag, size) in enumerate(filled)]

    def _drain_shared(self):
        key, pipe, in_flight = self._shared_active
        self._shared_active = None
        out = []
        for rec in pipe.flush():
            out += self._unpack_shared(rec, key, in_flight)
        return out

    @torch.no_grad()
    def submit_expressions(self, clip: torch.Tensor, token_ids, tags, original_size=None):
        """Streaming form for share_video=True: ONE clip [T,3,H,W] and the E expressions of it (token_ids: E tensors [1,L_e],
        tags: E tags).  The expressions fill the `group` slots of the shared-video pipeline -- E > group: ceil(E / group)
        replays of the staged clip; a part-filled replay runs with stale slots whose records are dropped -- and every replay
        runs the video side once.  Returns the list of result dicts that became available (those of the replay before, as
        submit does; drain() returns the rest), in the order the expressions were given, each what submit yields for
        (clip, that expression)."""
        if not (self.use_graphs and self.share_video):
            raise RuntimeError("submit_expressions() needs use_graphs=True and share_video=True")
        if len(token_ids) != len(tags) or not len(token_ids):
            raise ValueError("submit_expressions takes one tag per expression and at least one expression")
        self._check_weights()
        T, _, H, W = clip.shape
        ids, attns = self._pad_expressions(token_ids, self.pad_tokens_to)
        key = (T, H, W, ids[0].shape[-1])
        out = []
        if self._active is not None:
            out += self.drain()                                   # clips of the unshared stream are staged or in flight
        if self._shared_active is not None and self._shared_active[0] != key:
            out += self._drain_shared()                           # geometry change
        pipe = self._shared_pipeline(key)
        for at in range(0, len(ids), self.group):
            if at == 0:
                pipe.stage_video(clip)                            # the later replays of this call read the same static clip
            filled = []
            for s in range(min(self.group, len(ids) - at)):
                pipe.stage_inputs(ids[at + s], attns[at + s], slot=s)
                filled.append((tags[at + s], original_size))
            rec = pipe.replay()
            self.stats["shared_video_passes"] += 1
            self.stats["shared_expressions"] += len(filled)
            self.stats["stale_slots"] += self.group - len(filled)
            in_flight = self._shared_active[2] if self._shared_active is not None else []
            self._shared_active = (key, pipe, filled)
            if rec is not None and in_flight:
                if at + self.group < len(ids):                    # another replay of this call overwrites the record the results view
                    rec = rec.clone()
                out += self._unpack_shared(rec, key, in_flight)
        return out

    @torch.no_grad()
    def run_expressions(self, clip: torch.Tensor, token_ids, original_size=None):
        """Eager form for share_video=True (use_graphs=False): ONE clip and its E expressions through
        SOC.forward_expressions -> E result dicts, each what __call__ gives for (clip, that expression)."""
        if not self.share_video or self.use_graphs:
            raise RuntimeError("run_expressions() is the eager shared-video form: share_video=True, use_graphs=False")
        T, _, H, W = clip.shape
        ids, attns = self._pad_expressions(token_ids, None)       # eager: no graph geometry to keep, pad to the longest only
        ids = torch.cat(ids, 0)
        attn = torch.cat([torch.ones_like(ids[:1]) if a is None else a for a in attns], 0)
        samples = NestedTensor(clip[:, None], torch.zeros(T, 1, H, W, dtype=torch.bool, device=clip.device), unpadded=True)
        out = self.model.forward_expressions(samples, {"input_ids": ids, "attention_mask": attn},
                                             [[{"size": (H, W)}] for _ in range(T)])
        self.stats["shared_video_passes"] += 1
        self.stats["shared_expressions"] += ids.shape[0]
        results = []
        for e in range(ids.shape[0]):
            one = {"pred_cls": out["pred_cls"][:, e:e + 1], "pred_masks": out["pred_masks"][:, e:e + 1]}
            idx, masks = P.select_trajectory(one)
            res = {"query": idx, "mask_logits": masks, "pred_cls": one["pred_cls"][:, 0, :, 0], "record": None}
            if original_size is not None:
                self._masks_into(res, masks, original_size)
            results.append(res)
        return results

    @torch.no_grad()
    def forward_clip(self, clip: torch.Tensor, token_ids: torch.Tensor):
        """-> (reference output dict, packed record or None)"""
        T, _, H, W = clip.shape
        if self.use_graphs:
            self._check_weights()
            ids, attn = self._pad_tokens(token_ids)
            g = self.graph_for(T, H, W, ids.shape[-1])
            return g.run(clip, ids, attn), g.record
        samples = NestedTensor(clip[:, None], torch.zeros(T, 1, H, W, dtype=torch.bool, device=clip.device),
                               unpadded=True)
        ids = token_ids.view(1, -1)
        out = self.model(samples, None, {"input_ids": ids, "attention_mask": torch.ones_like(ids)},
                         [[{"size": (H, W)}] for _ in range(T)])
        return out, None

    @torch.no_grad()
    def __call__(self, clip: torch.Tensor, token_ids: torch.Tensor,
                 original_size: Optional[Sequence[int]] = None):
        """clip [T,3,H,W] (normalised, on the device), token_ids [1,L] -> dict with
        'query' (0-d int64 tensor), 'mask_logits' [T,H/4,W/4], 'pred_cls' [T,Q], and, when
        original_size=(H0,W0) is given, 'masks' bool [T,H0,W0] (packed_masks=True: 'masks_packed' uint8 [T,H0,RB] and
        'mask_size' instead)."""
        out, record = self.forward_clip(clip, token_ids)
        idx, masks = P.select_trajectory(out)
        res = {"query": idx, "mask_logits": masks, "pred_cls": out["pred_cls"][:, 0, :, 0], "record": record}
        if original_size is not None:
            self._masks_into(res, masks, original_size)
        return res


def load_checkpoint(model, path: str, require_text_encoder: bool = True):
    """The reference's on-disk contract (infer_refytb.py:143-156): `torch.load(path)["model_state_dict"]`, strict=False,
    the profiler's `total_params` / `total_ops` buffers ignored, anything else missing or unexpected printed.
    Returns (missing, unexpected) after that filter."""
    state = torch.load(path, map_location="cpu")["model_state_dict"]
    missing, unexpected = model.load_state_dict(state, strict=False)
    unexpected = [k for k in unexpected if not k.endswith(("total_params", "total_ops"))]
    if missing or unexpected:
        print(f"Missing Keys: {missing}\nUnexpected Keys: {unexpected}")
    # The drivers build the model with a randomly initialised RoBERTa (no download offline) and rely on the checkpoint to
    # overwrite it, as the reference's checkpoint overwrites its from_pretrained weights.  A checkpoint WITHOUT text_encoder.*
    # tensors would leave the random ones in place and write plausible-looking, wrong masks: refuse it.
    # position_ids is a derived buffer some transformers versions keep out of the state_dict.
    text_missing = [k for k in missing if k.startswith("text_encoder.") and not k.endswith("position_ids")]
    if text_missing and require_text_encoder:
        raise RuntimeError(f"{path}: the checkpoint has no weights for {len(text_missing)} text-encoder tensors "
                           f"(first: {text_missing[0]}); the model's text encoder is randomly initialised, so its masks would be "
                           "meaningless -- pass a checkpoint that carries text_encoder.*")
    return missing, unexpected


def load_tokenizer(path: str):
    """`RobertaTokenizerFast.from_pretrained(DIR)` (models/soc.py:104) -> tokenize(expression) -> int64 [1,L], encoded the
    way SOC.forward_text does it (padding='longest' over a batch of one = no padding)."""
    from .soc import encode_expressions, load_roberta_tokenizer
    hf = load_roberta_tokenizer(path)

    def tokenize(text):
        return encode_expressions(hf, [text])[0]
    tokenize.hf = hf
    return tokenize


def _run_jhmdb(a, dev, rank: int, world: int):
    """The JHMDB-Sentences evaluation (infer_jhmdb.py): eager forwards with valid_indices, K6c, the metrics dict."""
    from . import build_model, default_args, infer_jhmdb, synthetic_dataset
    from . import weights as W
    if a.make_synthetic and rank == 0:
        infer_jhmdb.make_synthetic(a.root, videos=a.make_synthetic, frames=max(a.frames, 4) + 4)
    args = default_args(a.backbone, text_encoder_random_init=True)
    args.dataset_name = "jhmdb_sentences"
    model, _, _ = build_model(args)
    if a.checkpoint:
        load_checkpoint(model, a.checkpoint)
    else:
        W.load_synthetic(model, 2023)
    tokenize = load_tokenizer(a.tokenizer) if a.tokenizer else synthetic_dataset.HashTokenizer()
    model = model.to(dev).eval()
    for _ in range(max(a.repeat, 1)):
        stats = infer_jhmdb.run(model, tokenize, a.root, a.out, rank, world, dev, samples_file=a.samples, seed=a.seed,
                                group=a.group, save_predictions=a.save_predictions)
    stats["samples_per_s"] = stats["samples"] / stats["seconds"]
    print(json.dumps({"rank": rank, "world": world, **stats}))


def _run_dataset(a):
    """infer_refytb.py / infer_davis.py `main`: one process per GPU over a static split of the videos
    (reference infer_refytb.py:84-109), no collective -- every rank writes its own PNGs."""
    from . import build_model, default_args, infer_davis, infer_refytb, synthetic_dataset
    from . import weights as W
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if a.gpus != world:
        raise RuntimeError(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if a.dataset == "jhmdb":
        return _run_jhmdb(a, dev, rank, world)
    if a.make_synthetic and rank == 0:
        expressions = 8 if a.dataset == "davis" else 3
        synthetic_dataset.make_dataset(a.root, videos=a.make_synthetic, frames=a.frames, expressions=expressions,
                                       n_words=a.words)
        if a.dataset == "davis" and a.eval_davis:
            synthetic_dataset.make_davis_annotations(a.root, a.eval_davis, objects=2, void=True)
        if a.eval_refytb:
            synthetic_dataset.make_refytb_annotations(a.root, "valid", objects=2, seed=0, void=True, out_root=a.eval_refytb)
    meta = os.path.join(a.root, "meta_expressions", "valid", "meta_expressions.json")
    for _ in range(600):                       # other ranks: the meta file is written last
        if os.path.exists(meta):
            break
        time.sleep(0.2)
    # The text encoder's architecture comes from the config; its weights from the checkpoint (a trained SOC checkpoint holds
    # every text_encoder.* tensor -- a gap would be printed as Missing Keys) or from the synthetic generator: no HuggingFace
    # download is needed either way (the reference's from_pretrained at build time is overwritten by its checkpoint as well).
    model, _, _ = build_model(default_args(a.backbone, text_encoder_random_init=True))
    if a.checkpoint:
        load_checkpoint(model, a.checkpoint)
    else:
        W.load_synthetic(model, 2023)
    if a.tokenizer:
        tokenize = load_tokenizer(a.tokenizer)
    else:
        tokenize = synthetic_dataset.HashTokenizer()
    driver = infer_refytb if a.dataset == "refytb" else infer_davis
    model = model.to(dev).eval()
    engine = ClipInferencer(model, dev, use_graphs=a.graphs, pad_tokens_to=32, group=a.group if a.graphs else 1,
                            packed_masks=a.packed_masks, share_video=a.share_video)   # shared across passes
    extra = {"packed_masks": True} if a.packed_masks else {}
    if a.share_video:
        extra.update(share_video=True)
    if a.eval_davis:
        if a.dataset != "davis":
            raise RuntimeError("--eval-davis scores the output of --dataset davis")
        extra.update(eval_root=a.eval_davis, eval_task=a.eval_task)
    if a.eval_refytb:
        extra.update(eval_root=a.eval_refytb)
    for _ in range(max(a.repeat, 1)):
        stats = driver.run(model, tokenize, a.root, a.out, rank, world, dev, engine=engine, **extra)
    stats["clips_per_s"] = stats["expressions"] / stats["seconds"]
    if "jf" in stats and "global" in stats["jf"]:
        jf = stats["jf"]
        print(" ".join(f"{h:>9}" for h in jf["measures"]))
        print(" ".join(f"{x:9.5f}" for x in jf["global"]))
    elif "jf" in stats:
        jf = stats["jf"]
        print(" " * 7 + " ".join(f"{h:>9}" for h in jf["measures"]))
        for name, row in [(f"anno_{i}", r) for i, r in enumerate(jf["per_annotator"])] + [("mean", jf["mean"])]:
            print(f"{name:>7} " + " ".join(f"{x:9.5f}" for x in row))
    print(json.dumps({"rank": rank, "world": world, **stats}))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--backbone", default="video-swin-t")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--orig", type=int, nargs=2, default=[720, 1280], help="original frame size for the output masks")
    ap.add_argument("--dataset", choices=["refytb", "davis", "jhmdb"], help="run a dataset driver instead of the clip stream")
    ap.add_argument("--root", help="dataset root (JPEGImages + meta_expressions, reference layout)")
    ap.add_argument("--out", help="output directory for the mask PNGs")
    ap.add_argument("--tokenizer", help="directory with RobertaTokenizerFast files (default: synthetic hash tokenizer)")
    ap.add_argument("--checkpoint", help="reference checkpoint (.pth with 'model_state_dict'); default: synthetic weights")
    ap.add_argument("--make-synthetic", type=int, default=0, metavar="N",
                    help="first write an N-video synthetic dataset (720x1280 JPEGs) under --root")
    ap.add_argument("--graphs", action="store_true", help="hipGraph replay per clip geometry in the dataset drivers")
    ap.add_argument("--group", type=int, default=None,
                    help="--graphs: consecutive clips of one geometry per launch group (each gets its single-clip result; clips of "
                         "different videos share a group when their geometry is the same; a remainder of fewer than half a group "
                         "leaves through the one-clip graph).  Default: 8 with --graphs, 1 without")
    ap.add_argument("--eval-davis", metavar="DIR",
                    help="--dataset davis: score the label maps against the DAVIS tree DIR (ImageSets, Annotations[_unsupervised]) on "
                         "the device and write the J&F CSVs into each anno_<a> directory; with --make-synthetic a synthetic "
                         "ground truth is written to DIR first")
    ap.add_argument("--eval-task", default="unsupervised", choices=["semi-supervised", "unsupervised"],
                    help="--eval-davis: the DAVIS task (the reference's eval_davis.py default: unsupervised)")
    ap.add_argument("--eval-refytb", metavar="DIR",
                    help="--dataset refytb: score every expression's masks against the tree DIR (valid/Annotations and a "
                         "meta_expressions.json whose expressions carry obj_id) on the device and write the per-expression J&F CSVs "
                         "into --out; with --make-synthetic a synthetic ground truth is written to DIR first")
    ap.add_argument("--packed-masks", action="store_true",
                    help="--dataset refytb: masks leave the GPU bit-packed (one bit per pixel, packed_masks.py) and the PNG files are "
                         "encoded from the bits; same files as without the flag")
    ap.add_argument("--share-video", action="store_true",
                    help="--dataset refytb / davis: all expressions of a video (davis: of a 36-frame chunk) go through the model in "
                         "one call that runs Video-Swin and the rest of the video side once for them; with --graphs they fill the "
                         "--group slots of the shared-video graph.  Same files as without the flag")
    ap.add_argument("--samples", metavar="FILE",
                    help="--dataset jhmdb: the samples to score, in the reference's metadata format (JSON rows of [video_id, "
                         "frame_path, masks_path, total_frames, query]; only the frame number of frame_path is used).  Without "
                         "it three frames per (video, query) are drawn from --seed and written to --out/samples.json; the "
                         "paper's numbers need the reference's own samples file")
    ap.add_argument("--seed", type=int, default=0, help="--dataset jhmdb: seed of the drawn samples")
    ap.add_argument("--save-predictions", action="store_true",
                    help="--dataset jhmdb: also write --out/predictions.json, COCO results of all queries of every sample with "
                         "uncompressed run-length counts")
    ap.add_argument("--words", type=int, default=0, help="--make-synthetic: fixed number of words per expression")
    ap.add_argument("--repeat", type=int, default=1, help="run the driver this many times, report the last (warm) pass")
    ap.add_argument("--gpus", "-ng", type=int, default=None,
                    help="GPUs of this node; >1 without an outer launcher starts one rank per GPU (reference -ng).  "
                         "Default: WORLD_SIZE under an outer launcher, 1 otherwise; an explicit value must equal WORLD_SIZE")
    a = ap.parse_args(argv)
    if a.packed_masks and a.dataset == "jhmdb":
        ap.error("--packed-masks applies to --dataset refytb (--dataset jhmdb writes no mask files, and its masks leave the "
                 "kernel bit-packed whatever the flag says)")
    if a.packed_masks and a.dataset != "refytb":
        ap.error("--packed-masks applies to --dataset refytb (the DAVIS driver writes label maps, which are not one-bit data)")
    if a.eval_refytb and a.dataset != "refytb":
        ap.error("--eval-refytb scores the output of --dataset refytb (--eval-davis is the flag of --dataset davis)")
    if a.share_video and not a.dataset:
        ap.error("--share-video applies to the dataset drivers (--dataset refytb | davis)")
    if a.share_video and a.dataset == "jhmdb":
        ap.error("--share-video applies to --dataset refytb | davis (a JHMDB-Sentences video has one expression: there is "
                 "nothing to share)")
    if a.eval_davis and a.dataset == "jhmdb":
        ap.error("--eval-davis scores the output of --dataset davis (--dataset jhmdb prints its own metrics)")
    if a.graphs and a.dataset == "jhmdb":
        ap.error("--graphs applies to --dataset refytb | davis (the centre-frame forward of --dataset jhmdb runs eagerly)")
    if (a.samples or a.save_predictions) and a.dataset != "jhmdb":
        ap.error("--samples and --save-predictions apply to --dataset jhmdb")
    if a.group is None:
        a.group = 8 if a.graphs else 1
    a.gpus_given = a.gpus is not None
    if a.gpus is None:
        a.gpus = int(os.environ["WORLD_SIZE"]) if CP.launched_as_rank() else 1
    return a


def main(argv=None):
    a = parse_args(argv)
    CP.rank_environment()           # before anything touches the GPU: the same process environment in both launch modes
    if a.gpus > 1 and not CP.launched_as_rank():
        # one process per GPU, started before this process touches the GPU (reference infer_refytb.py:84-109)
        import sys
        return CP.spawn_ranks(a.gpus, [sys.executable, "-m", "neurips2023_soc_amd.infer",
                                       *(sys.argv[1:] if argv is None else argv)])
    if a.dataset:
        return _run_dataset(a)
    import torch.distributed as dist
    from . import build_model, default_args
    from . import weights as W

    rank, local, world = CP.init_rank("cuda", expect_world=a.gpus)
    CP.pin_rank_cpus(rank, world)
    dev = torch.device("cuda", local)
    model, _, _ = build_model(default_args(a.backbone, text_encoder_random_init=True))
    W.load_synthetic(model, 2023)
    run = ClipInferencer(model.to(dev).eval(), dev)

    T, H, Wd, L = a.frames, a.height, a.width, 10
    mine = CP.shard_clips(a.clips, rank, world)
    n_local = -(-a.clips // world)
    hm, wm = -(-H // 4), -(-Wd // 4)
    records = torch.zeros(n_local, CP.record_size(T, 20, hm, wm), device=dev)
    fg = torch.zeros(n_local, device=dev)
    # synthetic stream: clip i / expression i from seeds, like tests/golden (seed 1 == golden clip)
    clips = [W.synthetic_clip(1 + i, T, H, Wd).pin_memory() for i in mine]
    ids = [W.synthetic_token_ids(1 + i, L).to(dev) for i in mine]
    from .clip_io import DoubleBufferedH2D
    feeder = DoubleBufferedH2D((T, 3, H, Wd), torch.float32, dev, depth=2)

    def run_local(out):
        # H2D inside the loop, like the reference (infer_refytb.py:206-212), but from pinned memory on a copy stream,
        # one clip ahead of the compute stream
        if clips:
            feeder.submit(clips[0])
        for slot, t in enumerate(ids):
            if slot + 1 < len(clips):
                feeder.submit(clips[slot + 1])
            res = run(feeder.acquire(), t, a.orig)
            out[slot].copy_(res["record"])
            fg[slot] = res["masks"].float().mean()
            feeder.release()

    timed = CP.timed_sharded_run(run_local, records, dev)             # the one collective sits inside
    gathered, dt = CP.interleave(timed["gathered"], a.clips), timed["seconds"]
    fgs = CP.interleave(CP.gather_results(fg[:, None]), a.clips)
    if rank == 0:
        qs = [int(gathered[i, 0].item()) for i in range(a.clips)]
        print(json.dumps({"clips": a.clips, "world": world, "ranks_seen": timed["ranks_seen"], "seconds": dt,
                          "clips_per_s": a.clips / dt,
                          "selected_queries": qs, "foreground_fraction": [round(float(v), 4) for v in fgs[:, 0]]}))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    raise SystemExit(main())
