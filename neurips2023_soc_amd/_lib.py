"""ctypes binding of libsoc_hip.so (include/soc_hip.h).  Fails loudly: there is no CPU or
PyTorch fallback for the four hot ops -- if the library is missing the product path raises."""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  -- loads the process's single HIP runtime before our library

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libsoc_hip.so")

EXPORTS = ("soc_hip_abi_version", "soc_hip_error_string", "soc_stream_cus", "soc_msda_fwd_f32", "soc_msda_fwd_f64",
           "soc_win_attn3d_f32", "soc_xattn_workspace_bytes", "soc_xattn_f32", "soc_dyn_mask_f32",
           "soc_add_layernorm_f32", "soc_msda_fused_fwd_f32", "soc_upsample_threshold_u8",
           "soc_linear_small_f32", "soc_linear_small_multi_f32", "soc_box_refine_f32",
           "soc_upsample_merge_labels_u8", "soc_resize_workspace_bytes", "soc_resize_normalize_u8_f32",
           "soc_msda_bwd_f32", "soc_msda_bwd_f64", "soc_groupnorm_tokens_workspace_bytes",
           "soc_groupnorm_tokens_f32", "soc_patch_merge_layernorm_f32", "soc_patch_embed_layernorm_f32", "soc_linear_act_f32",
           "soc_linear_act_multi_f32", "soc_ws_linear_f32", "soc_decoder_cross_attn_f32",
           "soc_row_mlp_f32", "soc_groupnorm_nchw_f32", "soc_upsample_add_nchw_f32",
           "soc_upsample_add_tokens_f32", "soc_conv3x3_tokens_f32", "soc_linear_split_packed_bytes",
           "soc_linear_split_pack_f32", "soc_row_stats_f32", "soc_linear_split_f32",
           "soc_mlp_split_packed_bytes", "soc_mlp_split_pack_f32",
           "soc_mlp_split_workspace_bytes", "soc_mlp_split_plan", "soc_mlp_split_max_hidden", "soc_mlp_split_f32", "soc_mlp_split_variant_f32",
           "soc_xs_linear_packed_bytes", "soc_xs_linear_pack_f32", "soc_xs_linear_plan", "soc_xs_linear_f32",
           "soc_small_attn_f32", "soc_select_pack_f32",
           "soc_davis_jf_workspace_bytes", "soc_davis_jf_counts_u8")
ABI_VERSION = 16
SOC_EINVAL = -1            # include/soc_hip.h: null pointer / non-positive dimension
SOC_EUNSUPPORTED = -2      # include/soc_hip.h: shape outside what the kernel is built for
SOC_EWORKSPACE = -4        # include/soc_hip.h: workspace too small

_lib = None


class SocHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SocHipError(
            f"{LIB_PATH} is missing: build it with `python -m neurips2023_soc_amd.build_ext` "
            "(hipcc --offload-arch=gfx950).  The SOC hot path has no CPU/PyTorch fallback.")
    from . import build_ext
    if build_ext.stale():
        # csrc/*.hip or include/*.h are newer than the .so: running it would test / time stale kernels.
        # Rebuild through a hipcc child process when the compiler is here, otherwise refuse.
        try:
            build_ext.build(verbose=False)
        except Exception as exc:
            raise SocHipError(f"{LIB_PATH} is older than its sources and could not be rebuilt ({exc}); "
                              "run `python -m neurips2023_soc_amd.build_ext`") from exc
    lib = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise SocHipError(f"libsoc_hip.so does not export {name}")
    p, i, f = C.c_void_p, C.c_int, C.c_float
    lib.soc_hip_abi_version.restype = i
    lib.soc_mlp_split_max_hidden.restype = i
    lib.soc_select_pack_f32.restype = i
    lib.soc_select_pack_f32.argtypes = [p, C.c_long, C.c_long, C.c_long, p, p, C.c_long, i, i, i, i, C.c_long, p]
    lib.soc_stream_cus.restype = i
    lib.soc_stream_cus.argtypes = [p]
    lib.soc_mlp_split_max_hidden.argtypes = [i]
    lib.soc_hip_error_string.restype = C.c_char_p
    lib.soc_hip_error_string.argtypes = [i]
    for fn in (lib.soc_msda_fwd_f32, lib.soc_msda_fwd_f64):
        fn.restype = i
        fn.argtypes = [p, p, p, p, p, p, i, i, i, i, i, i, i, p]
    for fn in (lib.soc_msda_bwd_f32, lib.soc_msda_bwd_f64):
        fn.restype = i
        fn.argtypes = [p] * 9 + [i] * 7 + [p]
    lib.soc_win_attn3d_f32.restype = i
    lib.soc_win_attn3d_f32.argtypes = [p, p, p, p] + [i] * 16 + [p]      # ... tab_w, split, stream
    lib.soc_xattn_workspace_bytes.restype = C.c_size_t
    lib.soc_xattn_workspace_bytes.argtypes = [i] * 5
    lib.soc_xattn_f32.restype = i
    lib.soc_xattn_f32.argtypes = [p, p, p, p, p, i, p, i, i, i, i, i, i, p, C.c_size_t, p]
    lib.soc_dyn_mask_f32.restype = i
    lib.soc_dyn_mask_f32.argtypes = [p, p, p, p, i, i, i, i, i, f, f, i, p]
    lib.soc_msda_fused_fwd_f32.restype = i
    lib.soc_msda_fused_fwd_f32.argtypes = [p, p, p, p, p, p, i, p, p, p, i, i, i, i, i, i, i, p]
    lib.soc_ws_linear_f32.restype = i
    lib.soc_ws_linear_f32.argtypes = [p, p, p, f, p, p, p, p, C.c_long, i, i, i, i, p]    # ... act, split, stream
    lib.soc_decoder_cross_attn_f32.restype = i
    lib.soc_decoder_cross_attn_f32.argtypes = [p, p, i, p, i, p, p, p, p, p] + [p] * 10 + [f, p] + [i] * 7 + [p]
    lib.soc_row_mlp_f32.restype = i
    lib.soc_row_mlp_f32.argtypes = [p, p, i, i, i, p, p, i, p, p, p, f, p, i, i, p]
    lib.soc_groupnorm_nchw_f32.restype = i
    lib.soc_groupnorm_nchw_f32.argtypes = [p, p, p, p, p, i, i, i, i, f, i, p]
    lib.soc_upsample_add_nchw_f32.restype = i
    lib.soc_upsample_add_nchw_f32.argtypes = [p, p, p, p, i, i, i, i, i, i, p]
    lib.soc_upsample_add_tokens_f32.restype = i
    lib.soc_upsample_add_tokens_f32.argtypes = [p, p, p, p, i, i, i, i, i, i, p]
    lib.soc_conv3x3_tokens_f32.restype = i
    lib.soc_conv3x3_tokens_f32.argtypes = [p, C.c_long, p, p, p, i, i, i, i, i, i, i, p]
    lib.soc_upsample_threshold_u8.restype = i
    lib.soc_upsample_threshold_u8.argtypes = [p, p, i, i, i, i, i, f, p]
    lib.soc_add_layernorm_f32.restype = i
    lib.soc_add_layernorm_f32.argtypes = [p, p, p, p, p, p, C.c_long, i, f, p]
    lib.soc_linear_small_f32.restype = i
    lib.soc_linear_small_f32.argtypes = [p, p, i, i, p, p, p, i, i, i, i, p]
    lib.soc_linear_small_multi_f32.restype = i
    lib.soc_linear_small_multi_f32.argtypes = [p, p, i, i, i, p, p, p, p, p, i, i, i, p]
    lib.soc_box_refine_f32.restype = i
    lib.soc_box_refine_f32.argtypes = [p, p, i, p, p, p, i, i, i, p]
    lib.soc_upsample_merge_labels_u8.restype = i
    lib.soc_upsample_merge_labels_u8.argtypes = [p, p, i, i, i, i, i, i, f, f, p]
    lib.soc_resize_workspace_bytes.restype = C.c_size_t
    lib.soc_resize_workspace_bytes.argtypes = [i] * 5
    lib.soc_resize_normalize_u8_f32.restype = i
    lib.soc_resize_normalize_u8_f32.argtypes = [p, p, p, i, i, i, i, i, p, p, i, p, p, i, p, p, p, C.c_size_t, p]
    lib.soc_groupnorm_tokens_workspace_bytes.restype = C.c_size_t
    lib.soc_groupnorm_tokens_workspace_bytes.argtypes = [i] * 4
    lib.soc_groupnorm_tokens_f32.restype = i
    lib.soc_groupnorm_tokens_f32.argtypes = [p, p, p, p, i, i, i, i, f, i, p, C.c_size_t, p]
    lib.soc_patch_merge_layernorm_f32.restype = i
    lib.soc_patch_merge_layernorm_f32.argtypes = [p, p, p, p, i, i, i, i, f, p]
    lib.soc_mlp_split_packed_bytes.restype = C.c_size_t
    lib.soc_mlp_split_packed_bytes.argtypes = [i, i]
    lib.soc_mlp_split_pack_f32.restype = i
    lib.soc_mlp_split_pack_f32.argtypes = [p, p, p, i, i, p]
    lib.soc_mlp_split_workspace_bytes.restype = C.c_size_t
    lib.soc_mlp_split_workspace_bytes.argtypes = [C.c_long, i, i, p]
    lib.soc_mlp_split_plan.restype = i
    lib.soc_mlp_split_plan.argtypes = [C.c_long, i, i, C.POINTER(i), C.POINTER(i), p]
    lib.soc_mlp_split_f32.restype = i
    lib.soc_mlp_split_f32.argtypes = [p, p, p, p, p, p, f, p, p, p, f, p, p, p, C.c_size_t, C.c_long, i, i, i, i, p]
    lib.soc_mlp_split_variant_f32.restype = i
    lib.soc_mlp_split_variant_f32.argtypes = [p, p, p, p, p, p, f, p, p, p, f, p, p, p, C.c_long, i, i, i, i, i, i, i, p]
    lib.soc_xs_linear_packed_bytes.restype = C.c_size_t
    lib.soc_xs_linear_packed_bytes.argtypes = [i, i]
    lib.soc_xs_linear_pack_f32.restype = i
    lib.soc_xs_linear_pack_f32.argtypes = [p, p, i, i, p]
    lib.soc_xs_linear_plan.restype = i
    lib.soc_xs_linear_plan.argtypes = [C.c_long, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i), p]
    lib.soc_xs_linear_f32.restype = i
    lib.soc_xs_linear_f32.argtypes = [p, p, p, p, p, f, p, p, C.c_long, i, i, i, i, i, p]
    lib.soc_patch_embed_layernorm_f32.restype = i
    lib.soc_patch_embed_layernorm_f32.argtypes = [p, p, p, p, p, p, i, i, i, i, f, p]
    lib.soc_linear_act_f32.restype = i
    lib.soc_linear_act_f32.argtypes = [p, p, p, p, i, i, i, i, p]
    lib.soc_linear_act_multi_f32.restype = i
    lib.soc_linear_act_multi_f32.argtypes = [p, p, i, p, p, p, p, i, i, i, p]
    lib.soc_linear_split_packed_bytes.restype = C.c_size_t
    lib.soc_linear_split_packed_bytes.argtypes = [i, i]
    lib.soc_linear_split_pack_f32.restype = i
    lib.soc_linear_split_pack_f32.argtypes = [p, p, i, i, p]
    lib.soc_row_stats_f32.restype = i
    lib.soc_row_stats_f32.argtypes = [p, p, C.c_long, i, f, p]
    lib.soc_linear_split_f32.restype = i
    lib.soc_linear_split_f32.argtypes = [p] * 10 + [i, C.c_long, i, i, i, i, p]
    lib.soc_small_attn_f32.restype = i
    lib.soc_small_attn_f32.argtypes = [p, p, p, p, p, i, i, i, i, f, C.c_long, C.c_long, p]
    lib.soc_davis_jf_workspace_bytes.restype = C.c_size_t
    lib.soc_davis_jf_workspace_bytes.argtypes = [i] * 5
    lib.soc_davis_jf_counts_u8.restype = i
    lib.soc_davis_jf_counts_u8.argtypes = [p, p, p] + [i] * 8 + [p, C.c_size_t, p]
    if lib.soc_hip_abi_version() != ABI_VERSION:
        raise SocHipError("libsoc_hip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().soc_hip_error_string(code).decode()
        raise SocHipError(f"{what}: {msg} (code {code})")
