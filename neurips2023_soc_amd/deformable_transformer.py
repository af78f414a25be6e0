"""Deformable transformer (3 enc + 3 dec layers) around K2/K3
(reference models/deformable_transformer.py:25-445, two_stage=False, box refinement on)."""
from __future__ import annotations

import copy

import torch
from torch import nn

from . import fused, hot_ops
from .fused import linear_relu
from .attention import HipMultiheadAttention
from .derived_cache import hold
from .ms_deform_attn import MSDeformAttn


def _add_norm(x, y, norm: nn.LayerNorm):
    """post-norm residual: LayerNorm(x + y) in one pass (K5)"""
    return hot_ops.add_layernorm(x, y, norm.weight, norm.bias, norm.eps, return_sum=False)[1]


class DeformableTransformerEncoderLayer(nn.Module):
    def __init__(self, d_model, d_ffn, n_levels, n_heads, n_points):
        super().__init__()
        self.self_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.norm1 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.norm2 = nn.LayerNorm(d_model)

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, padding_mask=None,
                pad_flag=None, out_tag=None):
        if fused.mlp_ok(src, self.linear1, self.linear2):
            # the shortcut rides in output_proj's epilogue; norm1, linear1 + ReLU + linear2, the shortcut norm1(.) and norm2 are ONE
            # K23 launch (whole rounds of the chip + a split tail): no LayerNorm pass in the layer
            s1, _, _ = self.self_attn(src, reference_points, src, spatial_shapes, level_start_index, padding_mask,
                                      pad_flag=pad_flag, return_sampling=False, query_pos=pos, residual=src)
            return hot_ops.mlp_split(s1, self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias, "relu",
                                     ln=(self.norm1.weight, self.norm1.bias, self.norm1.eps), residual=s1, residual_ln=True,
                                     post_ln=(self.norm2.weight, self.norm2.bias, self.norm2.eps),
                                     out=hot_ops.placed(out_tag, s1))
        a, _, _ = self.self_attn(src, reference_points, src, spatial_shapes, level_start_index, padding_mask,
                                 pad_flag=pad_flag, return_sampling=False, query_pos=pos)
        src = _add_norm(src, a, self.norm1)
        return _add_norm(src, fused.ffn_relu(src, self.linear1, self.linear2), self.norm2)


class DeformableTransformerEncoder(nn.Module):
    def __init__(self, layer, num_layers):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(num_layers)])
        self.num_layers = num_layers

    @staticmethod
    def get_reference_points(spatial_shapes, valid_ratios, device):
        """Pixel-centre grid of every level, normalised by the valid extent (reference :273-285).
        ``spatial_shapes`` may be a python list of (H, W) -- preferred: no device->host sync."""
        pts = []
        if torch.is_tensor(spatial_shapes):
            spatial_shapes = spatial_shapes.tolist()
        for lvl, (H_, W_) in enumerate(spatial_shapes):
            ys = torch.linspace(0.5, H_ - 0.5, H_, dtype=torch.float32, device=device)
            xs = torch.linspace(0.5, W_ - 0.5, W_, dtype=torch.float32, device=device)
            gy, gx = torch.meshgrid(ys, xs, indexing="ij")
            gy = gy.reshape(-1)[None] / (valid_ratios[:, None, lvl, 1] * H_)
            gx = gx.reshape(-1)[None] / (valid_ratios[:, None, lvl, 0] * W_)
            pts.append(torch.stack((gx, gy), -1))
        return torch.cat(pts, 1)[:, :, None] * valid_ratios[:, None]

    def forward(self, src, spatial_shapes, level_start_index, valid_ratios, pos=None, padding_mask=None,
                shapes_list=None, pad_flag=None, reference_points=None):
        ref = reference_points
        if ref is None:
            ref = self.get_reference_points(shapes_list if shapes_list is not None else spatial_shapes,
                                            valid_ratios, src.device)
        for layer in self.layers:       # the last layer's K23 launch writes into a placed buffer when the caller set one
            src = layer(src, pos, ref, spatial_shapes, level_start_index, padding_mask, pad_flag,
                        out_tag="encoder_memory" if layer is self.layers[-1] else None)
        return src


class DeformableTransformerDecoderLayer(nn.Module):
    def __init__(self, d_model, d_ffn, n_levels, n_heads, n_points):
        super().__init__()
        self.cross_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.norm1 = nn.LayerNorm(d_model)
        self.self_attn = HipMultiheadAttention(d_model, n_heads)
        self.norm2 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.norm3 = nn.LayerNorm(d_model)

    def forward(self, tgt, query_pos, reference_points, src, spatial_shapes, level_start_index, src_padding_mask=None,
                pad_flag=None, value=None):
        tgt = self.self_attn(tgt, tgt, tgt, query_add=query_pos, key_add=query_pos, batch_first=True,
                             post_norm=self.norm2)
        if (value is None and (src_padding_mask is None or pad_flag is not None)
                and hot_ops.decoder_cross_attn_supported(tgt, self.cross_attn, src, reference_points)):
            # K15: the whole block in one launch, value_proj applied to the sampled rows instead of the whole memory
            tgt = hot_ops.decoder_cross_attn(tgt, query_pos, reference_points, src, spatial_shapes, level_start_index,
                                             self.cross_attn, self.norm1, src_padding_mask, pad_flag)
            loc = w = None
        else:
            c, loc, w = self.cross_attn(tgt, reference_points, src, spatial_shapes, level_start_index,
                                        src_padding_mask, pad_flag=pad_flag, return_sampling=False,
                                        query_pos=query_pos, value=value)
            tgt = _add_norm(tgt, c, self.norm1)
        tgt = _add_norm(tgt, fused.apply(self.linear2, linear_relu(tgt, self.linear1)), self.norm3)
        return tgt, loc, w


class DeformableTransformerDecoder(nn.Module):
    def __init__(self, layer, num_layers, return_intermediate=False):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(num_layers)])
        self.num_layers, self.return_intermediate = num_layers, return_intermediate
        self.bbox_embed = None  # set by SOC to share the box heads (reference models/soc.py:95)
        self.class_embed = None

    def forward(self, tgt, reference_points, src, spatial_shapes, level_start_index, valid_ratios,
                query_pos=None, src_padding_mask=None, pad_flag=None, values=None):
        out = tgt
        inter, inter_refs = [], []
        ref_in = None
        for lid, layer in enumerate(self.layers):
            if ref_in is None:           # first layer, or no box refinement: scale by the valid ratios here
                if reference_points.shape[-1] == 4:
                    ref_in = reference_points[:, :, None] * torch.cat([valid_ratios, valid_ratios], -1)[:, None]
                else:
                    ref_in = reference_points[:, :, None] * valid_ratios[:, None]
            out, _, _ = layer(out, query_pos, ref_in, src, spatial_shapes, level_start_index, src_padding_mask,
                              pad_flag, value=None if values is None else values[lid])
            ref_in = None
            # (the reference's top-30 sample bookkeeping :383-389 feeds nothing in SOC.forward)
            if self.bbox_embed is not None:
                # K8: sigmoid(delta + inverse_sigmoid(ref)) and the next layer's ref_in in one launch
                reference_points, ref_in = hot_ops.box_refine(self.bbox_embed[lid](out), reference_points,
                                                              valid_ratios)
            if self.return_intermediate:
                inter.append(out)
                inter_refs.append(reference_points)
        if self.return_intermediate:
            return torch.stack(inter), torch.stack(inter_refs), None
        return out, reference_points, None


class DeformableTransformer(nn.Module):
    def __init__(self, d_model=256, nhead=8, num_encoder_layers=6, num_decoder_layers=6,
                 dim_feedforward=1024, dropout=0.1, activation="relu", return_intermediate_dec=False,
                 num_feature_levels=4, dec_n_points=4, enc_n_points=4, two_stage=False,
                 two_stage_num_proposals=300):
        super().__init__()
        if two_stage:
            raise NotImplementedError("two_stage=True is not on SOC's path (all shipped configs use False)")
        if activation != "relu":
            raise NotImplementedError("SOC builds the transformer with relu (reference :438)")
        self.d_model, self.nhead, self.num_feature_level = d_model, nhead, num_feature_levels
        enc = DeformableTransformerEncoderLayer(d_model, dim_feedforward, num_feature_levels, nhead, enc_n_points)
        self.encoder = DeformableTransformerEncoder(enc, num_encoder_layers)
        dec = DeformableTransformerDecoderLayer(d_model, dim_feedforward, num_feature_levels, nhead, dec_n_points)
        self.decoder = DeformableTransformerDecoder(dec, num_decoder_layers, return_intermediate_dec)
        self.level_embed = nn.Parameter(torch.empty(num_feature_levels, d_model))
        self.reference_points = nn.Linear(d_model, 2)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        for m in self.modules():
            if isinstance(m, MSDeformAttn):
                m._reset_parameters()
        nn.init.zeros_(self.reference_points.bias)
        nn.init.normal_(self.level_embed)

    def _shape_tensors(self, shapes, device):
        """[L,2] (H,W) int64 + [L] level starts on the device, cached per geometry: a host->device
        copy per forward would also be illegal inside a HIP-graph capture."""
        cache = self.__dict__.setdefault("_shape_cache", {})
        key = (shapes, str(device))
        if key not in cache:
            ss = torch.as_tensor(shapes, dtype=torch.long, device=device)
            cache[key] = (ss, torch.cat((ss.new_zeros(1), ss.prod(1).cumsum(0)[:-1])))
        return hold(cache[key])

    @staticmethod
    def get_valid_ratio(mask):
        _, H, W = mask.shape
        vh = (~mask[:, :, 0]).sum(1).float() / H
        vw = (~mask[:, 0, :]).sum(1).float() / W
        return torch.stack([vw, vh], -1)

    def _unpadded_constants(self, shapes, n, pos_embeds, device):
        """Everything encode() derives from the geometry alone when no frame is padded (~95 tiny
        launches, 0.45 ms at the BASELINE config): the all-False mask, valid ratios = 1, the K2 pad flag
        = 0, the encoder reference points and pos + level_embed.  Cached per (geometry, level_embed
        version), like the reference caches compute_mask per geometry (video_swin_transformer.py:316).
        The cache is bounded: the 18th distinct key drops the 17 entries before it.  That frees only what nobody holds -- a graph
        runner that was handed an entry during its warm-up and capture keeps it (derived_cache.keep_alive) for as long as the
        runner lives, whatever happens to the entry here."""
        cache = self.__dict__.setdefault("_unpadded_cache", {})
        key = (shapes, n, str(device), self.level_embed.data_ptr(), self.level_embed._version,
               tuple(p.data_ptr() for p in pos_embeds))
        if key not in cache:
            if len(cache) > 16:
                cache.clear()
            S = sum(h * w for h, w in shapes)
            ratios = torch.ones(n, len(shapes), 2, dtype=torch.float32, device=device)
            cache[key] = {
                "mask": torch.zeros(n, S, dtype=torch.bool, device=device),
                "ratios": ratios,
                "pad_flag": torch.zeros(1, dtype=torch.int32, device=device) if device.type == "cuda" else None,
                "ref": DeformableTransformerEncoder.get_reference_points(list(shapes), ratios, device),
                "pos": torch.cat([pe.flatten(2).transpose(1, 2) + self.level_embed[lvl].view(1, 1, -1)
                                  for lvl, pe in enumerate(pos_embeds)], 1),
            }
        return hold(cache[key])

    def encode(self, srcs, masks, pos_embeds, token_major=False, unpadded=False, maps=True):
        """Flatten the levels and run the deformable encoder.  Returns (memory maps of the 3 finest
        levels as '(b t) c h w', context for decode()).  Split from forward() so that SOC can run the
        FPN spatial decoder (needs only the maps) concurrently with the query decoder.
        ``token_major=True``: srcs are already '(b t) (h w) c' (what the fusion produces), which saves a
        layout round trip per level; masks / pos_embeds stay '(b t) [c] h w'.
        ``unpadded=True``: the caller vouches (host side) that every mask is all-False."""
        shapes = [tuple(m.shape[-2:]) for m in masks]
        src = torch.cat([s if token_major else s.flatten(2).transpose(1, 2) for s in srcs], 1)
        spatial_shapes, level_start = self._shape_tensors(tuple(shapes), src.device)
        if unpadded:
            const = self._unpadded_constants(tuple(shapes), src.shape[0], pos_embeds, src.device)
            mask, pos, ratios, pad_flag, ref = (const[k] for k in ("mask", "pos", "ratios", "pad_flag", "ref"))
        else:
            mask = torch.cat([m.flatten(1) for m in masks], 1)
            pos = torch.cat([pe.flatten(2).transpose(1, 2) + self.level_embed[lvl].view(1, 1, -1)
                             for lvl, pe in enumerate(pos_embeds)], 1)
            ratios = torch.stack([self.get_valid_ratio(m) for m in masks], 1)
            # one device-side flag "is there any padding" lets K2 skip the per-tap mask test without a
            # host sync
            pad_flag = mask.any().to(torch.int32).reshape(1) if mask.is_cuda else None
            ref = None
        memory = self.encoder(src, spatial_shapes, level_start, ratios, pos, mask, shapes_list=shapes,
                              pad_flag=pad_flag, reference_points=ref)
        ctx = (memory, spatial_shapes, level_start, ratios, mask, pad_flag, tuple(shapes))
        return (self.memory_maps(ctx) if maps else None), ctx

    def memory_maps(self, ctx):
        """The encoder output of the 3 finest levels as '(b t) c h w' maps (what the FPN spatial decoder reads)."""
        memory, shapes = ctx[0], ctx[6]
        n, _, c = memory.shape
        maps, at = [], 0
        for (h, w) in shapes[:self.num_feature_level - 1]:
            maps.append(memory[:, at:at + h * w].reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous())
            at += h * w
        return maps

    def decode(self, ctx, tgt, query_embed, values=None):
        """tgt [b,t,q,c], query_embed [q,c] -> hs [l,(b t),q,c], init_ref [(b t),q,2], inter_refs [l,(b t),q,4]"""
        memory, spatial_shapes, level_start, ratios, mask, pad_flag = ctx[:6]
        b, t, q, c = tgt.shape
        tgt = tgt.reshape(b * t, q, c)
        qpos = query_embed.unsqueeze(0).expand(b * t, -1, -1)
        ref = self.reference_points(query_embed).sigmoid().unsqueeze(0).expand(b * t, -1, -1)
        hs, inter_refs, _ = self.decoder(tgt, ref, memory, spatial_shapes, level_start, ratios, qpos, mask, pad_flag,
                                         values=values)
        return hs, ref, inter_refs

    def forward(self, srcs, tgt, masks, pos_embeds, query_embed=None):
        """srcs/masks/pos per level '(b t) c h w'; tgt [b,t,q,c]; query_embed [q,c]
        -> hs [l,(b t),q,c], memory maps, init_ref [(b t),q,2], inter_refs [l,(b t),q,4], None, None, None
        (return signature of the reference, models/deformable_transformer.py:132-220)"""
        maps, ctx = self.encode(srcs, masks, pos_embeds)
        hs, ref, inter_refs = self.decode(ctx, tgt, query_embed)
        return hs, maps, ref, inter_refs, None, None, None


def build_deforamble_transformer(args):  # (sic) name kept from the reference :430
    return DeformableTransformer(
        d_model=args["d_model"], nhead=args["nheads"], num_encoder_layers=args["enc_layers"],
        num_decoder_layers=args["dec_layers"], dim_feedforward=args["dim_feedforward"],
        dropout=args["dropout"], activation="relu", return_intermediate_dec=True,
        num_feature_levels=args["num_feature_levels"], dec_n_points=args["dec_n_points"],
        enc_n_points=args["enc_n_points"], two_stage=args["two_stage"],
        two_stage_num_proposals=args["num_queries"])
