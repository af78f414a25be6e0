"""Result selection / mask post-processing of the inference drivers.

select_trajectory + upsample_and_threshold restate infer_refytb.py:216-231;
ReferYoutubeVOSPostProcess mirrors models/postprocessing.py:193-234; merge_davis_objects the
multi-object argmax of infer_davis.py:264-272; A2DSentencesPostProcess models/postprocessing.py:10-55
(the centre-frame protocol of A2D-Sentences / JHMDB-Sentences, on K6c).
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import nn


def select_trajectory(outputs: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """B=1: (query index [], mask logits [T,h,w]) of the query with the best mean sigmoid score."""
    scores = outputs["pred_cls"][:, 0].sigmoid().mean(0).max(-1)[0]
    idx = scores.argmax(-1)
    return idx, outputs["pred_masks"][:, 0].index_select(1, idx.view(1))[:, 0]


def upsample_and_threshold(mask_logits: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """[T,h,w] logits -> bool [T,H0,W0] (bilinear, align_corners=False, sigmoid>0.5).
    On the GPU this is the fused HIP kernel K6; CPU tensors (host-side post-processing of gathered
    results) take the two torch ops the reference uses."""
    if mask_logits.is_cuda:
        from . import hot_ops
        return hot_ops.upsample_threshold(mask_logits, size)
    up = F.interpolate(mask_logits[None], size=tuple(size), mode="bilinear", align_corners=False)[0]
    return up.sigmoid() > 0.5


def upsample_and_threshold_packed(mask_logits: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """upsample_and_threshold with one BIT per pixel: [T,h,w] logits -> uint8 [T,H0,RB], the packed format of packed_masks.py
    (row_bytes(W0) bytes per row, pixel x = bit x % 8 of byte x // 8).  On the GPU the fused HIP kernel K6b; CPU tensors take
    the reference's two torch ops and pack()."""
    from . import packed_masks
    if mask_logits.is_cuda:
        return packed_masks.upsample_threshold_bits(mask_logits, size)
    return packed_masks.pack(upsample_and_threshold(mask_logits, size))


def merge_davis_objects(soft_masks: torch.Tensor, threshold: float = 0.5, background: float = 0.1) -> torch.Tensor:
    """soft_masks [O,T,H,W] sigmoid scores of O objects -> label map [T,H,W] (0 = background)."""
    m = torch.where(soft_masks < threshold, torch.zeros_like(soft_masks), soft_masks)
    bg = torch.full_like(m[:1], background)
    return torch.cat([bg, m], 0).argmax(0)


class ReferYoutubeVOSPostProcess(nn.Module):
    @torch.inference_mode()
    def forward(self, outputs, videos_metadata, samples_shape_with_padding):
        prob = outputs["pred_cls"].sigmoid().mean(0)          # [b, nq, k]
        best = prob.max(-1)[0].argmax(-1)                      # [b]
        masks = outputs["pred_masks"].permute(1, 0, 2, 3, 4)   # b t nq h w
        b = masks.shape[0]
        masks = masks[torch.arange(b, device=masks.device), :, best]
        masks = F.interpolate(masks, size=samples_shape_with_padding, mode="bilinear", align_corners=False)
        masks = masks.sigmoid() > 0.5
        preds = []
        for vm, meta in zip(masks, videos_metadata):
            rh, rw = meta["resized_frame_size"]
            vm = vm[:, :rh, :rw].unsqueeze(1)
            vm = F.interpolate(vm.float(), size=meta["original_frame_size"], mode="nearest")
            preds.append({**meta, "pred_masks": vm.to(torch.uint8).cpu()})
        return preds


class A2DSentencesPostProcess(nn.Module):
    """The centre-frame post-processor of A2D-Sentences / JHMDB-Sentences (reference models/postprocessing.py:10-55): per
    annotated frame the scores of all queries and their masks at the frame's original size.

    outputs: 'pred_cls' [t,b,Q,1] and 'pred_masks' [t*b,Q,h,w] (the reference's caller flattens it; [t,b,Q,h,w] is flattened
    here).  -> per frame {'scores': [Q] = pred_cls[..., 0].sigmoid(), 'masks': float32 [Q,1,oh,ow] of zeros and ones,
    'rle_masks': per query {'size': [oh, ow], 'counts': [...]}}.  On CUDA tensors the masks are K6c's (center_frame.py: one
    launch for all frames and queries); CPU tensors take the reference's torch ops.

    'counts' are UNCOMPRESSED COCO run lengths -- column-major runs, the first one of zeros -- built on the host from the
    packed bits.  The compressed string form the reference stores is pycocotools' encoding, which is not available here and
    is not produced; pycocotools' frPyObjects turns the uncompressed form into it."""

    @torch.inference_mode()
    def forward(self, outputs, resized_padded_sample_size, resized_sample_sizes, orig_sample_sizes):
        from . import center_frame as CF
        from . import packed_masks
        scores = outputs["pred_cls"].flatten(0, 1)[..., 0].sigmoid()
        pred_masks = outputs["pred_masks"]
        if pred_masks.dim() == 5:
            pred_masks = pred_masks.flatten(0, 1)
        padded = tuple(int(v) for v in resized_padded_sample_size)
        resized = [tuple(int(v) for v in s) for s in resized_sample_sizes]
        original = [tuple(int(v) for v in s) for s in orig_sample_sizes]
        Q = pred_masks.shape[1]
        masks, packed = [], []
        if pred_masks.is_cuda:
            bits, _ = CF.center_frame_bits(pred_masks.float(), padded, resized, original, masks=True)
            host = bits.cpu()
            for n, (oh, ow) in enumerate(original):
                packed.append(CF.sample_masks(host, original, Q, n).numpy())
                masks.append(packed_masks.unpack(CF.sample_masks(bits, original, Q, n), ow).unsqueeze(1).float())
        else:
            up = F.interpolate(pred_masks, size=padded, mode="bilinear", align_corners=False).sigmoid() > 0.5
            for f_masks, (rh, rw), (oh, ow) in zip(up, resized, original):
                m = F.interpolate(f_masks[:, :rh, :rw].unsqueeze(1).float(), size=(oh, ow), mode="nearest")
                masks.append(m)
                packed.append(packed_masks.pack(m[:, 0].numpy()))
        rles = [[{"size": [oh, ow], "counts": CF.rle_counts(plane, (oh, ow))} for plane in planes]
                for planes, (oh, ow) in zip(packed, original)]
        return [{"scores": s, "masks": m, "rle_masks": r} for s, m, r in zip(scores, masks, rles)]


def build_postprocessors(dataset_name: str):
    """reference models/soc.py:648-660; the COCO pre-training post-processors are not built."""
    if dataset_name in ("a2d_sentences", "jhmdb_sentences"):
        return A2DSentencesPostProcess()
    if dataset_name in ("ref_youtube_vos", "joint"):
        return ReferYoutubeVOSPostProcess()
    if dataset_name == "davis":
        return None
    raise NotImplementedError(f"post-processor for {dataset_name!r} is outside the inference hot path "
                              "(COCO pre-training evaluation: SURVEY.md section 2, out of scope)")
