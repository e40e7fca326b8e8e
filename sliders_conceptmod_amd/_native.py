"""ctypes binding of libsmi_hip.so (include/smi.h).  PyTorch is used only to own device memory and streams:
tensors are passed as raw device pointers.  There is NO fallback: if the library is missing or fails to load, every
entry point raises (the product path never computes on the CPU)."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMI_LIB") or os.path.join(_HERE, "libsmi_hip.so")  # SMI_LIB: A/B runs of tools/ against another build
SMI_MAX_LEVELS = 8
DTYPE_CODE = {torch.float16: 0, torch.bfloat16: 1}


class SmiError(RuntimeError):
    pass


class UNetConfigC(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("in_channels", C.c_int), ("out_channels", C.c_int), ("n_levels", C.c_int),
        ("block_out_channels", C.c_int * SMI_MAX_LEVELS), ("down_has_attn", C.c_int * SMI_MAX_LEVELS),
        ("up_has_attn", C.c_int * SMI_MAX_LEVELS), ("layers_per_block", C.c_int),
        ("transformer_layers", C.c_int * SMI_MAX_LEVELS), ("num_heads", C.c_int * SMI_MAX_LEVELS),
        ("mid_transformer_layers", C.c_int), ("cross_attention_dim", C.c_int), ("norm_num_groups", C.c_int),
        ("use_linear_projection", C.c_int), ("addition_embed", C.c_int), ("addition_time_embed_dim", C.c_int),
        ("projection_class_embeddings_input_dim", C.c_int),
    ]


class VaeConfigC(C.Structure):
    _fields_ = [("dtype", C.c_int), ("in_channels", C.c_int), ("latent_channels", C.c_int), ("n_levels", C.c_int),
                ("block_out_channels", C.c_int * SMI_MAX_LEVELS), ("layers_per_block", C.c_int),
                ("norm_num_groups", C.c_int), ("no_post_quant_conv", C.c_int)]


class ClipConfigC(C.Structure):
    _fields_ = [("dtype", C.c_int), ("vocab_size", C.c_int), ("hidden_size", C.c_int), ("num_layers", C.c_int),
                ("num_heads", C.c_int), ("intermediate_size", C.c_int), ("max_positions", C.c_int),
                ("hidden_act", C.c_int), ("projection_dim", C.c_int)]


class ClipVisionConfigC(C.Structure):
    _fields_ = [("dtype", C.c_int), ("hidden_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int),
                ("intermediate_size", C.c_int), ("image_size", C.c_int), ("patch_size", C.c_int),
                ("hidden_act", C.c_int), ("projection_dim", C.c_int), ("image_mean", C.c_float * 3),
                ("image_std", C.c_float * 3)]


class LpipsConfigC(C.Structure):
    _fields_ = [("dtype", C.c_int), ("channels", C.c_int * 5)]


class MMDiTConfigC(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("dtype", "patch_size", "in_channels", "out_channels", "num_layers", "num_heads",
                                       "attention_head_dim", "joint_attention_dim", "pooled_projection_dim",
                                       "pos_embed_max_size", "context_len", "dual_attention_layers", "qk_norm")]


class FluxConfigC(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("dtype", "in_channels", "patch_size", "num_layers", "num_single_layers", "num_heads",
                                       "attention_head_dim", "joint_attention_dim", "pooled_projection_dim",
                                       "guidance_embeds")] + [("axes_dims_rope", C.c_int * 3), ("context_len", C.c_int),
                                                              ("rope_theta", C.c_float)]


class T5ConfigC(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("dtype", "vocab_size", "d_model", "d_kv", "num_heads", "d_ff", "num_layers",
                                       "rel_buckets", "rel_max_distance", "max_tokens")] + [("eps", C.c_float)]


class WeightC(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int), ("shape", C.c_int64 * 4)]


class LoraSiteC(C.Structure):
    _fields_ = [("target", C.c_char_p), ("off_down", C.c_int64), ("off_up", C.c_int64), ("rank", C.c_int),
                ("scale", C.c_float), ("off_dora", C.c_int64)]


class WgradJobC(C.Structure):
    """include/smi.h smi_wgrad_job: one entry of the grouped weight-gradient job table (test entry point)."""
    _fields_ = [("X", C.c_void_p), ("P", C.c_void_p), ("dW", C.c_void_p), ("row_scale", C.c_void_p),
                ("ldx", C.c_int64), ("ldp", C.c_int64), ("so_r", C.c_int64), ("so_k", C.c_int64),
                ("M", C.c_int), ("K", C.c_int), ("r", C.c_int), ("seg_cols", C.c_int), ("rows_per_sample", C.c_int),
                ("alpha", C.c_float), ("m_begin", C.c_int), ("conv_tap", C.c_int), ("Hin", C.c_int), ("Win", C.c_int),
                ("Hout", C.c_int), ("Wout", C.c_int), ("conv_stride", C.c_int), ("conv_ups", C.c_int)]


class AttnArgsC(C.Structure):
    """include/smi.h smi_attn_args: one attention launch with explicit leading dimensions (test entry point)."""
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p), ("lse", C.c_void_p),
                ("d_o", C.c_void_p), ("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p), ("delta", C.c_void_p),
                ("stream", C.c_void_p),
                ("ldq", C.c_int64), ("ldk", C.c_int64), ("ldv", C.c_int64), ("ldo", C.c_int64), ("lddo", C.c_int64),
                ("lddq", C.c_int64), ("lddk", C.c_int64), ("lddv", C.c_int64),
                ("dtype", C.c_int), ("b", C.c_int), ("h", C.c_int), ("nq", C.c_int), ("nk", C.c_int), ("d", C.c_int),
                ("scale", C.c_float), ("causal", C.c_int), ("sel_xs", C.c_int), ("sel_fused", C.c_int)]


class AttnRanC(C.Structure):
    """include/smi.h smi_attn_ran: what an smi_op_attention_ex_* call launched."""
    _fields_ = [("dp", C.c_int), ("form", C.c_int), ("n_launches", C.c_int), ("family", C.c_int * 4), ("chain", C.c_int)]


class NormArgsC(C.Structure):
    """include/smi.h smi_norm_args: one GroupNorm / LayerNorm forward (+ backward on a sub-range) (test entry point)."""
    _fields_ = [("x", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("y", C.c_void_p), ("dy", C.c_void_p),
                ("add", C.c_void_p), ("dx", C.c_void_p), ("scratch", C.c_void_p), ("stream", C.c_void_p),
                ("dtype", C.c_int), ("nb", C.c_int), ("hw", C.c_int), ("c", C.c_int), ("g", C.c_int), ("eps", C.c_float),
                ("silu", C.c_int), ("bwd_n0", C.c_int), ("sel_fused", C.c_int)]


class NormRanC(C.Structure):
    """include/smi.h smi_norm_ran: what an smi_op_groupnorm_ex / smi_op_layernorm_ex call launched."""
    _fields_ = [("form", C.c_int), ("chunks", C.c_int), ("slots", C.c_int), ("nv", C.c_int), ("r", C.c_int)]


class DoraSiteC(C.Structure):
    """include/smi.h smi_dora_site: one DoRA Linear of the per-kernel DoRA entry points."""
    _fields_ = [("W", C.c_void_p), ("off_down", C.c_int64), ("off_up", C.c_int64), ("off_dora", C.c_int64),
                ("dW", C.c_void_p), ("dWt", C.c_void_p), ("cnorm", C.c_void_p), ("r", C.c_int), ("nseg", C.c_int),
                ("K", C.c_int), ("cs", C.c_int), ("scale", C.c_float)]


class LoraPrepSiteC(C.Structure):
    """include/smi.h smi_lora_prep_site: one site of the 16-bit shadow-operand preparation."""
    _fields_ = [("off_down", C.c_int64), ("off_up", C.c_int64), ("dst_down", C.c_int64), ("dst_up", C.c_int64),
                ("r", C.c_int), ("nseg", C.c_int), ("K", C.c_int), ("cs", C.c_int), ("rows_pad", C.c_int), ("conv", C.c_int),
                ("dst_gw", C.c_int64)]


class LoraStackJobC(C.Structure):
    """include/smi.h smi_lora_stack_job: one (site, slider) block of the rank-stacked flat buffers."""
    _fields_ = [("src_down", C.c_void_p), ("src_up", C.c_void_p), ("dst_down", C.c_void_p), ("dst_up", C.c_void_p),
                ("row_len", C.c_int64), ("r", C.c_int), ("c0", C.c_int), ("R", C.c_int), ("n_out", C.c_int),
                ("coef", C.c_float), ("reserved", C.c_int)]


class ProdigyHyperC(C.Structure):
    """include/smi.h smi_prodigy_hyper: Prodigy's hyper-parameters, beta3 resolved."""
    _fields_ = [(k, C.c_double) for k in ("lr", "beta1", "beta2", "beta3", "eps", "weight_decay", "d0", "d_coef",
                                          "growth_rate")] + [("decouple", C.c_int), ("use_bias_correction", C.c_int),
                                                             ("safeguard_warmup", C.c_int)]


_lib = None

_SIGS = {
    "smi_last_error": (C.c_char_p, []),
    "smi_workspace_bytes": (C.c_int, [C.POINTER(UNetConfigC), C.POINTER(LoraSiteC), C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "smi_create": (C.c_int, [C.POINTER(UNetConfigC), C.POINTER(WeightC), C.c_int, C.POINTER(LoraSiteC), C.c_int,
                             C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                             C.POINTER(C.c_void_p)]),
    "smi_unet_forward_batched": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p]),
    "smi_unet_forward_multi": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_void_p]),
    "smi_unet_forward_compose": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                           C.POINTER(C.c_float), C.c_void_p]),
    "smi_lora_stack": (C.c_int, [C.POINTER(LoraStackJobC), C.c_int, C.c_void_p, C.c_void_p]),
    "smi_destroy": (None, [C.c_void_p]),
    "smi_weights_bytes": (C.c_int, [C.POINTER(UNetConfigC), C.POINTER(LoraSiteC), C.c_int, C.POINTER(C.c_size_t)]),
    "smi_arena_bytes": (C.c_int, [C.POINTER(UNetConfigC), C.POINTER(LoraSiteC), C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "smi_replan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "smi_engine_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "smi_vae_workspace_bytes": (C.c_int, [C.POINTER(VaeConfigC), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "smi_vae_create": (C.c_int, [C.POINTER(VaeConfigC), C.POINTER(WeightC), C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "smi_vae_encode": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "smi_vae_decoder_workspace_bytes": (C.c_int, [C.POINTER(VaeConfigC), C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(C.c_size_t)]),
    "smi_vae_decoder_create": (C.c_int, [C.POINTER(VaeConfigC), C.POINTER(WeightC), C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "smi_vae_decode": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smi_clip_workspace_bytes": (C.c_int, [C.POINTER(ClipConfigC), C.c_int, C.POINTER(C.c_size_t)]),
    "smi_clip_create": (C.c_int, [C.POINTER(ClipConfigC), C.POINTER(WeightC), C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                  C.c_void_p, C.POINTER(C.c_void_p)]),
    "smi_clip_encode": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 5),
    "smi_clip_encode_layers": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 6),
    "smi_t5_workspace_bytes": (C.c_int, [C.POINTER(T5ConfigC), C.c_int, C.POINTER(C.c_size_t)]),
    "smi_t5_create": (C.c_int, [C.POINTER(T5ConfigC), C.POINTER(WeightC), C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                C.c_void_p, C.POINTER(C.c_void_p)]),
    "smi_t5_encode": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "smi_t5_relative_buckets": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "smi_t5_lora_workspace_bytes": (C.c_int, [C.POINTER(T5ConfigC), C.POINTER(LoraSiteC), C.c_int, C.c_int,
                                              C.POINTER(C.c_size_t)]),
    "smi_t5_lora_create": (C.c_int, [C.POINTER(T5ConfigC), C.POINTER(WeightC), C.c_int, C.POINTER(LoraSiteC), C.c_int,
                                     C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "smi_t5_forward_lora": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.POINTER(C.c_float), C.c_int] +
                            [C.c_void_p] * 2),
    "smi_t5_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smi_clip_lora_workspace_bytes": (C.c_int, [C.POINTER(ClipConfigC), C.POINTER(LoraSiteC), C.c_int, C.c_int,
                                                C.POINTER(C.c_size_t)]),
    "smi_clip_lora_create": (C.c_int, [C.POINTER(ClipConfigC), C.POINTER(WeightC), C.c_int, C.POINTER(LoraSiteC), C.c_int,
                                       C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "smi_clip_forward_lora": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(C.c_float), C.c_int] +
                              [C.c_void_p] * 4),
    "smi_clip_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smi_clip_vision_workspace_bytes": (C.c_int, [C.POINTER(ClipVisionConfigC), C.c_int, C.POINTER(C.c_size_t)]),
    "smi_clip_vision_create": (C.c_int, [C.POINTER(ClipVisionConfigC), C.POINTER(WeightC), C.c_int, C.c_int, C.c_void_p,
                                         C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "smi_clip_vision_encode": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4),
    "smi_clip_logits": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                  C.c_void_p]),
    "smi_lpips_workspace_bytes": (C.c_int, [C.POINTER(LpipsConfigC), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "smi_lpips_create": (C.c_int, [C.POINTER(LpipsConfigC), C.POINTER(WeightC), C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "smi_lpips_distance": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.POINTER(C.c_void_p)]),
    "smi_mmdit_workspace_bytes": (C.c_int, [C.POINTER(MMDiTConfigC), C.POINTER(LoraSiteC), C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.POINTER(C.c_size_t)]),
    "smi_mmdit_create": (C.c_int, [C.POINTER(MMDiTConfigC), C.POINTER(WeightC), C.c_int, C.POINTER(LoraSiteC), C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "smi_mmdit_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)] + [C.c_void_p] * 4 +
                          [C.POINTER(C.c_float), C.c_void_p]),
    "smi_mmdit_train_workspace_bytes": (C.c_int, [C.POINTER(MMDiTConfigC), C.POINTER(LoraSiteC), C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.POINTER(C.c_size_t)]),
    "smi_mmdit_train_create": (C.c_int, [C.POINTER(MMDiTConfigC), C.POINTER(WeightC), C.c_int, C.POINTER(LoraSiteC), C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                         C.POINTER(C.c_void_p)]),
    "smi_mmdit_forward_save": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)] + [C.c_void_p] * 4 +
                               [C.POINTER(C.c_float), C.c_void_p]),
    "smi_mmdit_backward": (C.c_int, [C.c_void_p] * 4),
    "smi_flux_workspace_bytes": (C.c_int, [C.POINTER(FluxConfigC), C.POINTER(LoraSiteC), C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.POINTER(C.c_size_t)]),
    "smi_flux_create": (C.c_int, [C.POINTER(FluxConfigC), C.POINTER(WeightC), C.c_int, C.POINTER(LoraSiteC), C.c_int,
                                  C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "smi_flux_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)] +
                         [C.c_void_p] * 4 + [C.POINTER(C.c_float), C.c_void_p]),
    "smi_flux_train_workspace_bytes": (C.c_int, [C.POINTER(FluxConfigC), C.POINTER(LoraSiteC), C.c_int, C.c_int, C.c_int,
                                                 C.c_int, C.POINTER(C.c_size_t)]),
    "smi_flux_train_create": (C.c_int, [C.POINTER(FluxConfigC), C.POINTER(WeightC), C.c_int, C.POINTER(LoraSiteC), C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.POINTER(C.c_void_p)]),
    "smi_flux_forward_save": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)] +
                              [C.c_void_p] * 4 + [C.POINTER(C.c_float), C.c_void_p]),
    "smi_flux_backward": (C.c_int, [C.c_void_p] * 4),
    "smi_unet_forward": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p]),
    "smi_unet_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smi_unet_backward_tail": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smi_unet_ctx_grad_bytes": (C.c_int, [C.POINTER(UNetConfigC), C.POINTER(LoraSiteC), C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "smi_unet_ctx_grad_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "smi_unet_ctx_grad": (C.c_int, [C.c_void_p, C.c_int]),
    "smi_unet_backward_ctx": (C.c_int, [C.c_void_p] * 5),
    "smi_unet_pooled_grad_bytes": (C.c_int, [C.POINTER(UNetConfigC), C.POINTER(LoraSiteC), C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "smi_unet_pooled_grad_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "smi_unet_pooled_grad": (C.c_int, [C.c_void_p, C.c_int]),
    "smi_unet_backward_cond": (C.c_int, [C.c_void_p] * 6),
    "smi_nulltext_loss": (C.c_int, [C.c_void_p] * 4 + [C.c_float] * 3 + [C.c_int64] + [C.c_void_p] * 4),
    "smi_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "smi_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int64)]),
    "smi_cfg_combine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    "smi_slider_loss": (C.c_int, [C.c_void_p] * 4 + [C.c_float, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]),
    "smi_clip_adamw": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] + [C.c_float] * 5 + [C.c_int, C.c_float, C.c_void_p,
                                                                                    C.c_void_p]),
    "smi_clip_lion": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_double] * 4 + [C.c_float, C.c_void_p, C.c_void_p]),
    "smi_prodigy_init": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_double, C.c_void_p, C.c_void_p]),
    "smi_clip_prodigy": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.POINTER(ProdigyHyperC), C.c_float, C.c_void_p,
                                                      C.c_void_p, C.c_void_p]),
    "smi_sched_step": (C.c_int, [C.c_void_p] * 3 + [C.c_float] * 3 + [C.c_int64, C.c_void_p]),
    "smi_op_gemm_scratch": (C.c_int, [C.c_void_p, C.c_size_t]),
    "smi_op_gemm": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "smi_op_gemm_rows": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int,
                                   C.c_void_p]),
    "smi_op_gemm_epilogue": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 4 +
                             [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 3 +
                             [C.c_float] + [C.c_int] * 3 + [C.POINTER(C.c_int), C.c_void_p]),
    "smi_op_conv3x3": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 10 +
                       [C.c_void_p]),
    "smi_op_conv3x3_ex": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 12 +
                          [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                           C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p]),
    "smi_op_upconv_phase": (C.c_int, [C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 6 + [C.POINTER(C.c_int), C.c_void_p]),
    "smi_set_upconv_phase": (C.c_int, [C.c_int]),
    "smi_op_attention_fwd": (C.c_int, [C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_float, C.c_void_p]),
    "smi_op_attention_bwd": (C.c_int, [C.c_int] + [C.c_void_p] * 10 + [C.c_int] * 5 + [C.c_float, C.c_void_p]),
    "smi_op_attention_ex_fwd": (C.c_int, [C.POINTER(AttnArgsC), C.POINTER(AttnRanC)]),
    "smi_op_attention_ex_bwd": (C.c_int, [C.POINTER(AttnArgsC), C.POINTER(AttnRanC)]),
    "smi_op_attention_causal_fwd": (C.c_int, [C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_int64] * 4 +
                                    [C.c_float, C.c_void_p]),
    "smi_op_attention_causal_bwd": (C.c_int, [C.c_int] + [C.c_void_p] * 10 + [C.c_int] * 5 + [C.c_int64] * 8 +
                                    [C.c_float, C.c_void_p]),
    "smi_op_attention_bias_fwd": (C.c_int, [C.c_int] + [C.c_void_p] * 6 + [C.c_int64] + [C.c_int] * 4 + [C.c_int64] * 4 +
                                  [C.c_float, C.c_void_p]),
    "smi_op_rmsnorm": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "smi_op_gated_gelu_tanh": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "smi_op_t5_bias_table": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]),
    "smi_op_attention_bias_bwd": (C.c_int, [C.POINTER(AttnArgsC), C.c_void_p, C.c_int64, C.POINTER(AttnRanC)]),
    "smi_op_rmsnorm_bwd": (C.c_int, [C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "smi_op_gated_gelu_tanh_bwd": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int64, C.c_int, C.c_void_p]),
    "smi_op_act": (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_void_p]),
    "smi_op_groupnorm": (C.c_int, [C.c_int] + [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_float, C.c_int, C.c_void_p]),
    "smi_op_layernorm": (C.c_int, [C.c_int] + [C.c_void_p] * 7 + [C.c_int] * 2 + [C.c_float, C.c_void_p]),
    "smi_op_groupnorm_ex": (C.c_int, [C.POINTER(NormArgsC), C.POINTER(NormRanC), C.POINTER(NormRanC)]),
    "smi_op_layernorm_ex": (C.c_int, [C.POINTER(NormArgsC), C.POINTER(NormRanC), C.POINTER(NormRanC)]),
    "smi_op_pool2x2_sum": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "smi_op_colsum_floats": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "smi_op_colsum": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_float, C.c_void_p]),
    "smi_op_timestep_embed": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "smi_op_softmax_rows": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "smi_op_adaln_modulate": (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_int64, C.c_int, C.c_int, C.c_float,
                                                                                       C.c_void_p]),
    "smi_op_gate_residual": (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int,
                                                                      C.c_void_p]),
    "smi_op_adaln_modulate_bwd": (C.c_int, [C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_int64, C.c_int, C.c_void_p]),
    "smi_op_gate_residual_bwd": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int,
                                                                          C.c_void_p]),
    "smi_op_joint_rows_pack": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]),
    "smi_op_joint_rows_split": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]),
    "smi_op_sd3_patchify": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "smi_op_sd3_add_pos": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p]),
    "smi_op_sd3_unpatchify": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "smi_op_qk_norm_rope": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 3 +
                            [C.c_int] * 6 + [C.c_float, C.c_void_p]),
    "smi_op_gelu_tanh_cols": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                                        C.c_void_p]),
    "smi_op_flux_unpack": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "smi_op_qk_norm_rope_bwd": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] +
                                [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_float, C.c_void_p]),
    "smi_op_gelu_tanh_cols_bwd": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                            C.c_int64, C.c_int, C.c_void_p]),
    "smi_op_flux_unpack_bwd": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "smi_op_chan_mix": (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_void_p]),
    "smi_op_conv3x3_small": (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p]),
    "smi_op_nchw_to_nhwc": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_float, C.c_void_p]),
    "smi_op_nchw_to_nhwc_scaled": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]),
    "smi_op_geglu": (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_void_p]),
    "smi_op_gemm_geglu": (C.c_int, [C.c_int] + [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "smi_op_lora_down": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]),
    "smi_op_lora_skinny": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]),
    "smi_op_lora_skinny_cols": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 3 +
                                [C.c_void_p]),
    "smi_op_lora_wgrad": (C.c_int, [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_float, C.c_void_p,
                                                                                   C.c_void_p]),
    "smi_op_lora_wgrad_jobs_floats": (C.c_int, [C.POINTER(WgradJobC), C.c_int, C.POINTER(C.c_size_t)]),
    "smi_op_lora_wgrad_jobs": (C.c_int, [C.c_int, C.POINTER(WgradJobC), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "smi_op_dora_prep": (C.c_int, [C.c_int, C.POINTER(DoraSiteC), C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                   C.c_void_p, C.c_void_p]),
    "smi_op_dora_grads_floats": (C.c_int, [C.POINTER(DoraSiteC), C.POINTER(C.c_size_t)]),
    "smi_op_dora_grads": (C.c_int, [C.c_int, C.POINTER(DoraSiteC)] + [C.c_void_p] * 5 + [C.c_float, C.c_void_p,
                                                                                        C.c_void_p, C.c_size_t,
                                                                                        C.c_void_p]),
    "smi_op_lora_prep": (C.c_int, [C.c_int, C.POINTER(LoraPrepSiteC), C.c_int] + [C.c_void_p] * 5),
    "smi_op_transpose_scaled": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_int, C.c_void_p]),
    "smi_op_grad_scale": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "smi_op_cast_f32": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "smi_op_row_scale_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "smi_op_col_scale_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p]),
}

EXPORTED_SYMBOLS = sorted(_SIGS)


def lib():
    """Loads the shared library (once).  Raises SmiError if it has not been built -- no silent fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SmiError(f"{LIB_PATH} not found: build it with `python -m sliders_conceptmod_amd.build` "
                           f"(the HIP extension is mandatory; there is no CPU fallback)")
        try:
            l = C.CDLL(LIB_PATH)
        except OSError as e:
            raise SmiError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().smi_last_error()
        raise SmiError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_config(cfg, dtype: torch.dtype) -> UNetConfigC:
    """cfg: sliders_conceptmod_amd.unet.UNetConfig (the diffusers public config values)."""
    c = UNetConfigC()
    c.dtype = DTYPE_CODE[dtype]
    c.in_channels = cfg.in_channels
    c.out_channels = cfg.out_channels
    n = len(cfg.block_out_channels)
    c.n_levels = n
    for i in range(n):
        c.block_out_channels[i] = cfg.block_out_channels[i]
        c.down_has_attn[i] = int(cfg.down_block_types[i] == "CrossAttnDownBlock2D")
        c.up_has_attn[i] = int(cfg.up_block_types[i] == "CrossAttnUpBlock2D")
        c.transformer_layers[i] = cfg.transformer_layers_per_block[i]
        c.num_heads[i] = cfg.num_attention_heads[i]
    c.layers_per_block = cfg.layers_per_block
    c.mid_transformer_layers = cfg.mid_block_transformer_layers or cfg.transformer_layers_per_block[-1]
    c.cross_attention_dim = cfg.cross_attention_dim
    c.norm_num_groups = cfg.norm_num_groups
    c.use_linear_projection = int(cfg.use_linear_projection)
    c.addition_embed = int(cfg.addition_embed_type == "text_time")
    c.addition_time_embed_dim = cfg.addition_time_embed_dim
    c.projection_class_embeddings_input_dim = cfg.projection_class_embeddings_input_dim
    return c


def make_sites(sites: Sequence[dict]):
    """sites: [{'target': str, 'off_down': int, 'off_up': int, 'rank': int, 'scale': float}]"""
    arr = (LoraSiteC * max(1, len(sites)))()
    keep = []
    for i, s in enumerate(sites):
        b = s["target"].encode()
        keep.append(b)
        arr[i].target = b
        arr[i].off_down = s["off_down"]
        arr[i].off_up = s["off_up"]
        arr[i].rank = s["rank"]
        arr[i].scale = s["scale"]
        arr[i].off_dora = s.get("off_dora", -1)
    return arr, keep


def workspace_bytes(cfg_c: UNetConfigC, sites: Sequence[dict], batch: int, h: int, w: int, ctx_len: int,
                    batch_adapted: Optional[int] = None) -> int:
    arr, _keep = make_sites(sites)
    out = C.c_size_t(0)
    ba = batch if batch_adapted is None else batch_adapted
    check(lib().smi_workspace_bytes(C.byref(cfg_c), arr, len(sites), batch, ba, h, w, ctx_len, C.byref(out)),
          "smi_workspace_bytes")
    return out.value


def arena_bytes(cfg_c: UNetConfigC, sites: Sequence[dict], batch: int, h: int, w: int, ctx_len: int,
                batch_adapted: Optional[int] = None) -> int:
    arr, _keep = make_sites(sites)
    out = C.c_size_t(0)
    ba = batch if batch_adapted is None else batch_adapted
    check(lib().smi_arena_bytes(C.byref(cfg_c), arr, len(sites), batch, ba, h, w, ctx_len, C.byref(out)),
          "smi_arena_bytes")
    return out.value


class _EngineBase:
    """What the six engine wrappers share: the smi_engine `handle`, the `workspace` tensor it lives in, the weight
    tensors it borrows (kept alive for as long as the wrapper), and their release."""

    handle = None

    def _create(self, prefix: str, cfg_c, shape: tuple, state: dict, dtype: torch.dtype, device):
        """smi_<prefix>workspace_bytes(cfg, *shape) -> workspace on `device` -> smi_<prefix>create(cfg, weights, *shape)."""
        size_fn, create_fn = f"smi_{prefix}workspace_bytes", f"smi_{prefix}create"
        out = C.c_size_t(0)
        check(getattr(lib(), size_fn)(C.byref(cfg_c), *shape, C.byref(out)), size_fn)
        self.workspace = torch.empty(out.value, dtype=torch.uint8, device=device)
        warr, self._keep = _weight_table(state, dtype, self.workspace.device)
        handle = C.c_void_p()
        with torch.cuda.device(self.workspace.device):
            check(getattr(lib(), create_fn)(C.byref(cfg_c), warr, len(state), *shape, ptr(self.workspace), out.value,
                                            stream_ptr(), C.byref(handle)), create_fn)
        self.handle = handle

    def close(self):
        if self.handle:
            lib().smi_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine(_EngineBase):
    """Owns one smi_engine plus the torch tensors backing its workspace.

    The packed weights are shape-independent; `plan(batch, batch_adapted, h, w, ctx_len)` switches the engine to
    another shape by pointing it at another activation arena (smi_replan) -- no weight is re-packed and no GEMM tile is
    re-tuned for shapes already seen.  A small LRU of arenas keeps the `dynamic_resolution` buckets
    (T/train_util.py:1085-1097) resident; MAX_PLANS bounds it."""

    MAX_PLANS = 4

    def __init__(self, cfg, dtype: torch.dtype, state: dict, sites: Sequence[dict], batch: int, h: int, w: int,
                 ctx_len: int, device, batch_adapted: Optional[int] = None):
        self.cfg_c = make_config(cfg, dtype)
        self.dtype = dtype
        self.batch, self.h, self.w, self.ctx_len = batch, h, w, ctx_len
        self.batch_adapted = batch if batch_adapted is None else batch_adapted
        self.sites = list(sites)
        sarr, _keep = make_sites(sites)
        self._create("", self.cfg_c, (sarr, len(sites), batch, self.batch_adapted, h, w, ctx_len), state, dtype, device)
        self.stream = torch.cuda.current_stream().cuda_stream
        self._home = (batch, self.batch_adapted, h, w, ctx_len)  # the shape the creation workspace was sized for
        self._plans = {}                                         # shape -> arena tensor (LRU, most recent last)
        self._ctx_buf = None     # smi_unet_ctx_grad_attach buffer of the current shape (None: not attached)
        self._ctx_on = False
        self._pool_buf = None    # smi_unet_pooled_grad_attach buffer of the current shape
        self._pool_on = False

    def plan(self, batch: int, batch_adapted: int, h: int, w: int, ctx_len: int):
        """Make (batch, batch_adapted, h, w, ctx_len) the engine's current shape (no-op when it already is)."""
        cur = (self.batch, self.batch_adapted, self.h, self.w, self.ctx_len)
        want = (batch, batch_adapted, h, w, ctx_len)
        if want == cur:
            return
        arena = None
        if want != self._home:
            arena = self._plans.pop(want, None)
            if arena is None:
                nbytes = arena_bytes(self.cfg_c, self.sites, batch, h, w, ctx_len, batch_adapted)
                while len(self._plans) >= self.MAX_PLANS:
                    self._plans.pop(next(iter(self._plans)))
                arena = torch.empty(nbytes, dtype=torch.uint8, device=self.workspace.device)
            self._plans[want] = arena
        check(lib().smi_replan(self.handle, batch, batch_adapted, h, w, ctx_len, ptr(arena),
                               0 if arena is None else arena.numel()), "smi_replan")
        self.batch, self.batch_adapted, self.h, self.w, self.ctx_len = want
        self._ctx_buf, self._ctx_on = None, False  # smi_replan detaches the context-gradient buffer
        self._pool_buf, self._pool_on = None, False  # ... and the pooled-gradient buffer

    def _attach_grad_buffer(self, what: str) -> torch.Tensor:
        """Sizes (smi_unet_{what}_grad_bytes), allocates and attaches (smi_unet_{what}_grad_attach) the gradient buffer
        `what` ("ctx" / "pooled") of the current shape; the caller keeps the tensor it returns alive."""
        size_fn, attach_fn = f"smi_unet_{what}_grad_bytes", f"smi_unet_{what}_grad_attach"
        sarr, _keep = make_sites(self.sites)
        out = C.c_size_t(0)
        check(getattr(lib(), size_fn)(C.byref(self.cfg_c), sarr, len(self.sites), self.batch, self.batch_adapted, self.h,
                                      self.w, self.ctx_len, C.byref(out)), size_fn)
        buf = torch.empty(out.value, dtype=torch.uint8, device=self.workspace.device)
        with torch.cuda.device(self.workspace.device):
            check(getattr(lib(), attach_fn)(self.handle, ptr(buf), out.value), attach_fn)
        return buf

    def set_ctx_grad(self, on: bool):
        """Saving forwards from here on also differentiate the context of their adapted samples (smi_unet_ctx_grad); the
        extra buffer (transposed k|v weights + a larger saved-pass arena) is attached on first use for the current shape."""
        on = bool(on)
        if on and self._ctx_buf is None:
            self._ctx_buf = self._attach_grad_buffer("ctx")
        if on != self._ctx_on:
            check(lib().smi_unet_ctx_grad(self.handle, int(on)), "smi_unet_ctx_grad")
            self._ctx_on = on
            if not on:
                self._pool_on = False  # the engine turns the pooled gradient off with the context gradient

    def set_pooled_grad(self, on: bool):
        """Saving forwards that differentiate the context also differentiate the pooled embedding text_embeds of their
        adapted samples (smi_unet_pooled_grad; SD-XL only).  Call after set_ctx_grad(True); the extra buffer (the transposed
        grouped time_emb_proj weight + a saved-pass arena that is larger again) is attached on first use for the shape."""
        on = bool(on)
        if on and self._pool_buf is None:
            if self._ctx_buf is None:
                raise SmiError("set_pooled_grad(True) needs set_ctx_grad(True) first: the pooled-embedding gradient rides "
                               "on the context gradient's pass")
            self._pool_buf = self._attach_grad_buffer("pooled")
        if on != self._pool_on:
            check(lib().smi_unet_pooled_grad(self.handle, int(on)), "smi_unet_pooled_grad")
            self._pool_on = on

    def backward_cond(self, d_eps: torch.Tensor, d_down: Optional[torch.Tensor], d_up: Optional[torch.Tensor],
                      d_ctx: torch.Tensor, d_text_embeds: torch.Tensor):
        """smi_unet_backward_cond: backward_ctx of a pass saved under set_pooled_grad(True) that also WRITES
        d(loss)/d(text_embeds) of the adapted samples into d_text_embeds (fp32 [n_adapted, P])."""
        check(lib().smi_unet_backward_cond(self.handle, ptr(d_eps), ptr(d_down), ptr(d_up), ptr(d_ctx), ptr(d_text_embeds)),
              "smi_unet_backward_cond")

    def backward_ctx(self, d_eps: torch.Tensor, d_down: Optional[torch.Tensor], d_up: Optional[torch.Tensor],
                     d_ctx: torch.Tensor):
        """smi_unet_backward_ctx: the backward of a pass saved under set_ctx_grad(True); WRITES d(loss)/d(ctx) of the
        adapted samples into d_ctx (fp32 [n_adapted, ctx_len, D]); d_down / d_up may be None without an adaptor."""
        check(lib().smi_unet_backward_ctx(self.handle, ptr(d_eps), ptr(d_down), ptr(d_up), ptr(d_ctx)),
              "smi_unet_backward_ctx")

    def stats(self) -> dict:
        out = (C.c_int64 * 4)()
        check(lib().smi_engine_stats(self.handle, out), "smi_engine_stats")
        return {"pack_launches": out[0], "replans": out[1], "tape_generation": out[2], "weights_bytes": out[3]}

    def tape_generation(self) -> int:
        return self.stats()["tape_generation"] if self.handle else 0

    def forward(self, sample: torch.Tensor, timestep: float, ctx: torch.Tensor, text_embeds, time_ids, lora_down,
                lora_up, multiplier, save: bool, n_adapted: Optional[int] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """n_adapted: the LAST n_adapted samples get the LoRA delta and are differentiated (default: all).
        `multiplier`: one float, or a sequence of n_adapted floats (one adaptor multiplier per adapted sample,
        smi_unet_forward_multi).  `out`: an fp32 tensor of the sample's shape to write eps into (default: a new one)."""
        n = sample.shape[0]
        na = min(n, self.batch_adapted) if n_adapted is None else n_adapted
        eps = out if out is not None else torch.empty(sample.shape, dtype=torch.float32, device=sample.device)
        if isinstance(multiplier, (list, tuple)):
            if len(multiplier) != na:
                raise SmiError(f"{len(multiplier)} multipliers for {na} adapted samples")
            arr = (C.c_float * na)(*[float(m) for m in multiplier])
            check(lib().smi_unet_forward_multi(self.handle, n, na, ptr(sample), float(timestep), ptr(ctx),
                                               ptr(text_embeds), ptr(time_ids), ptr(lora_down), ptr(lora_up), arr,
                                               int(save), ptr(eps)), "smi_unet_forward_multi")
            return eps
        check(lib().smi_unet_forward_batched(self.handle, n, na, ptr(sample), float(timestep), ptr(ctx),
                                             ptr(text_embeds), ptr(time_ids), ptr(lora_down), ptr(lora_up),
                                             float(multiplier), int(save), ptr(eps)), "smi_unet_forward_batched")
        return eps

    def forward_compose(self, sample: torch.Tensor, timestep: float, ctx: torch.Tensor, text_embeds, time_ids, lora_down,
                        lora_up, ranks: Sequence[int], multipliers: Sequence[Sequence[float]],
                        n_adapted: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """smi_unet_forward_compose: `forward` with a stacked adaptor (compose.SliderStack) and one multiplier per
        (adapted sample, slider) -- `multipliers`: n_adapted rows of len(ranks) floats.  Inference only (nothing saved)."""
        n = sample.shape[0]
        na = min(n, self.batch_adapted) if n_adapted is None else n_adapted
        k = len(ranks)
        if len(multipliers) != na or any(len(row) != k for row in multipliers):
            raise SmiError(f"multipliers must be {na} rows (adapted samples) of {k} floats (sliders)")
        eps = out if out is not None else torch.empty(sample.shape, dtype=torch.float32, device=sample.device)
        rk = (C.c_int * max(k, 1))(*[int(r) for r in ranks])
        arr = (C.c_float * max(na * k, 1))(*[float(m) for row in multipliers for m in row])
        check(lib().smi_unet_forward_compose(self.handle, n, na, ptr(sample), float(timestep), ptr(ctx), ptr(text_embeds),
                                             ptr(time_ids), ptr(lora_down), ptr(lora_up), k, rk, arr, ptr(eps)),
              "smi_unet_forward_compose")
        return eps

    def backward(self, d_eps: torch.Tensor, d_down: torch.Tensor, d_up: torch.Tensor):
        check(lib().smi_unet_backward(self.handle, ptr(d_eps), ptr(d_down), ptr(d_up)), "smi_unet_backward")

    def backward_tail(self, d_eps_live: torch.Tensor, d_down: torch.Tensor, d_up: torch.Tensor):
        """Backward over the LAST d_eps_live.shape[0] adapted samples of the saved pass; the caller promises that the
        gradient of the other adapted samples' output is exactly zero (smi_unet_backward_tail)."""
        check(lib().smi_unet_backward_tail(self.handle, int(d_eps_live.shape[0]), ptr(d_eps_live), ptr(d_down),
                                           ptr(d_up)), "smi_unet_backward_tail")

    PROF_CLASSES = ("gemm", "conv", "attention", "norm", "elementwise", "lora")

    def profile_enable(self, on: bool):
        check(lib().smi_profile_enable(self.handle, int(on)), "smi_profile_enable")

    def profile_read(self) -> dict:
        n = len(self.PROF_CLASSES)
        ms, fl, by = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
        la = (C.c_int64 * n)()
        check(lib().smi_profile_read(self.handle, ms, fl, by, la), "smi_profile_read")
        return {k: {"ms": ms[i], "flops": fl[i], "bytes": by[i], "launches": la[i]}
                for i, k in enumerate(self.PROF_CLASSES)}


def nulltext_loss(eps_u, eps_c, x_t, target, guidance_scale: float, c_x: float, c_eps: float, loss_out, d_eps_u, scratch):
    """smi_nulltext_loss on caller-owned fp32 tensors (loss_out [1], d_eps_u like eps_u or None, scratch >= 256 floats):
    no allocation, no synchronisation."""
    check(lib().smi_nulltext_loss(ptr(eps_u), ptr(eps_c), ptr(x_t), ptr(target), float(guidance_scale), float(c_x),
                                  float(c_eps), eps_u.numel(), ptr(loss_out), ptr(d_eps_u), ptr(scratch), stream_ptr()),
          "smi_nulltext_loss")


def cast_f32(src: torch.Tensor, dst: torch.Tensor):
    """smi_op_cast_f32: dst (float16 / bfloat16) = src (fp32), same number of elements, a multiple of 8."""
    check(lib().smi_op_cast_f32(DTYPE_CODE[dst.dtype], ptr(src), ptr(dst), src.numel(), stream_ptr()), "smi_op_cast_f32")


def cfg_combine(eps_pair: torch.Tensor, guidance_scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """smi_cfg_combine: out = u + g (t - u) for the contiguous fp32 CFG-doubled batch eps_pair = [u ; t].  `out`: an fp32
    tensor of the half batch to write into (default: a new one).  No synchronisation."""
    if out is None:
        out = torch.empty((eps_pair.shape[0] // 2,) + tuple(eps_pair.shape[1:]), dtype=torch.float32,
                          device=eps_pair.device)
    check(lib().smi_cfg_combine(ptr(eps_pair), ptr(out), out.numel(), float(guidance_scale), stream_ptr()),
          "smi_cfg_combine")
    return out


def slider_loss(target, positive, neutral, negative, sign_eta: float, loss_out, d_target, scratch):
    """smi_slider_loss on caller-owned fp32 tensors (loss_out [1], d_target like target, scratch >= 256 floats):
    PromptEmbedsPair.loss with sign_eta = +eta (enhance) / -eta (erase) and its gradient.  No allocation, no
    synchronisation."""
    check(lib().smi_slider_loss(ptr(target), ptr(positive), ptr(neutral), ptr(negative), float(sign_eta), target.numel(),
                                ptr(loss_out), ptr(d_target), ptr(scratch), stream_ptr()), "smi_slider_loss")


def clip_adamw(param, grad, exp_avg, exp_avg_sq, lr: float, step: int, scratch, betas=(0.9, 0.999), eps=1e-8,
               weight_decay=1e-2, max_grad_norm=0.0):
    """smi_clip_adamw on flat fp32 tensors: clip_grad_norm_(max_grad_norm) (0: no clipping), then one torch.optim.AdamW
    step (decoupled weight decay).  scratch: >= 1025 floats.  No allocation, no synchronisation."""
    check(lib().smi_clip_adamw(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr),
                               float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step),
                               float(max_grad_norm), ptr(scratch), stream_ptr()), "smi_clip_adamw")


def adam_step(param, grad, exp_avg, exp_avg_sq, lr: float, step: int, scratch, beta1=0.9, beta2=0.999, eps=1e-8):
    """One torch.optim.Adam step on flat fp32 tensors: clip_adamw with weight_decay 0 and no clipping."""
    clip_adamw(param, grad, exp_avg, exp_avg_sq, lr, step, scratch, (beta1, beta2), eps, 0.0, 0.0)


def clip_lion(param, grad, exp_avg, lr: float, scratch, betas=(0.9, 0.99), weight_decay=0.0, max_grad_norm=0.0):
    """smi_clip_lion on flat fp32 tensors: clip_grad_norm_(max_grad_norm) (0: no clipping), then one Lion step.  scratch:
    >= 1025 floats.  No allocation, no synchronisation."""
    check(lib().smi_clip_lion(ptr(param), ptr(grad), ptr(exp_avg), param.numel(), float(lr), float(betas[0]),
                              float(betas[1]), float(weight_decay), float(max_grad_norm), ptr(scratch), stream_ptr()),
          "smi_clip_lion")


PRODIGY_STATE_DOUBLES = 8  # include/smi.h smi_prodigy_init: d, d_max, d_numerator, k, dlr, d (new), skip, reserved


def prodigy_hyper(lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0, decouple=True,
                  use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0,
                  growth_rate=float("inf")) -> ProdigyHyperC:
    """smi_prodigy_hyper from the package's keyword arguments (beta3 None -> sqrt(beta2))."""
    b3 = float(betas[1]) ** 0.5 if beta3 is None else float(beta3)
    return ProdigyHyperC(float(lr), float(betas[0]), float(betas[1]), b3, float(eps), float(weight_decay), float(d0),
                         float(d_coef), float(growth_rate), int(bool(decouple)), int(bool(use_bias_correction)),
                         int(bool(safeguard_warmup)))


def prodigy_init(param, p0, exp_avg, exp_avg_sq, s, state, d0: float = 1e-6):
    """smi_prodigy_init: p0 = param, zero moments, `state` (PRODIGY_STATE_DOUBLES float64 on the device) = a fresh group."""
    assert state.dtype == torch.float64 and state.numel() >= PRODIGY_STATE_DOUBLES
    check(lib().smi_prodigy_init(ptr(param), ptr(p0), ptr(exp_avg), ptr(exp_avg_sq), ptr(s), param.numel(), float(d0),
                                 ptr(state), stream_ptr()), "smi_prodigy_init")


def clip_prodigy(param, grad, p0, exp_avg, exp_avg_sq, s, state, scratch, hyper: ProdigyHyperC, max_grad_norm=0.0):
    """smi_clip_prodigy on flat fp32 tensors: clip_grad_norm_(max_grad_norm) (0: no clipping), then one Prodigy step with
    d and k on the device.  scratch: >= 3073 floats.  No allocation, no synchronisation."""
    check(lib().smi_clip_prodigy(ptr(param), ptr(grad), ptr(p0), ptr(exp_avg), ptr(exp_avg_sq), ptr(s), param.numel(),
                                 C.byref(hyper), float(max_grad_norm), ptr(state), ptr(scratch), stream_ptr()),
          "smi_clip_prodigy")


def _weight_table(state: dict, dtype, device):
    warr = (WeightC * len(state))()
    keep = []
    for i, (k, v) in enumerate(state.items()):
        if v.dtype != dtype or not v.is_contiguous() or v.device != device:
            raise SmiError(f"weight {k}: expected contiguous {dtype} on {device}")
        nb = k.encode()
        keep.append((nb, v))
        warr[i].name = nb
        warr[i].data = v.data_ptr()
        warr[i].ndim = v.ndim
        for d in range(v.ndim):
            warr[i].shape[d] = v.shape[d]
    return warr, keep


class VaeEngine(_EngineBase):
    """AutoencoderKL encoder on the HIP engine for one image size (smi_vae_*): image -> posterior moments."""

    def __init__(self, cfg, dtype: torch.dtype, state: dict, batch: int, h: int, w: int, device):
        self.cfg_c, self.batch, self.h, self.w = vae_config_c(cfg, dtype), batch, h, w
        self.latent_channels = cfg.latent_channels
        self.down = 2 ** (len(cfg.block_out_channels) - 1)
        self._create("vae_", self.cfg_c, (batch, h, w), state, dtype, device)

    def moments(self, image: torch.Tensor) -> torch.Tensor:
        n = image.shape[0]
        out = torch.empty((n, 2 * self.latent_channels, self.h // self.down, self.w // self.down), dtype=torch.float32,
                          device=image.device)
        check(lib().smi_vae_encode(self.handle, n, ptr(image), ptr(out)), "smi_vae_encode")
        return out


def vae_config_c(cfg, dtype: torch.dtype) -> VaeConfigC:
    c = VaeConfigC()
    c.dtype = DTYPE_CODE[dtype]
    c.in_channels, c.latent_channels = cfg.in_channels, cfg.latent_channels
    c.n_levels = len(cfg.block_out_channels)
    for i, v in enumerate(cfg.block_out_channels):
        c.block_out_channels[i] = v
    c.layers_per_block, c.norm_num_groups = cfg.layers_per_block, cfg.norm_num_groups
    c.no_post_quant_conv = int(not getattr(cfg, "use_post_quant_conv", True))
    return c


CLIP_ACT = {"quick_gelu": 0, "gelu": 1}


def clip_config_c(cfg, dtype: torch.dtype) -> ClipConfigC:
    if cfg.hidden_act not in CLIP_ACT:
        raise SmiError(f"CLIP hidden_act '{cfg.hidden_act}' is not built (quick_gelu / gelu)")
    c = ClipConfigC()
    c.dtype = DTYPE_CODE[dtype]
    c.vocab_size, c.hidden_size, c.num_layers = cfg.vocab_size, cfg.hidden_size, cfg.num_hidden_layers
    c.num_heads, c.intermediate_size = cfg.num_attention_heads, cfg.intermediate_size
    c.max_positions, c.hidden_act = cfg.max_position_embeddings, CLIP_ACT[cfg.hidden_act]
    c.projection_dim = cfg.projection_dim or 0
    return c


def vae_decoder_workspace_bytes(cfg, dtype: torch.dtype, batch: int, h: int, w: int) -> int:
    """smi_vae_decoder_workspace_bytes: a host-only dry run (no GPU needed); raises SmiError on a refused shape."""
    out = C.c_size_t(0)
    check(lib().smi_vae_decoder_workspace_bytes(C.byref(vae_config_c(cfg, dtype)), batch, h, w, C.byref(out)),
          "smi_vae_decoder_workspace_bytes")
    return out.value


class VaeDecoderEngine(_EngineBase):
    """AutoencoderKL decoder on the HIP engine for one image size (smi_vae_decoder_*): latents -> image (+ uint8)."""

    def __init__(self, cfg, dtype: torch.dtype, state: dict, batch: int, h: int, w: int, device):
        self.cfg_c, self.batch, self.h, self.w = vae_config_c(cfg, dtype), batch, h, w
        self.latent_channels, self.out_channels = cfg.latent_channels, cfg.in_channels
        self.down = 2 ** (len(cfg.block_out_channels) - 1)
        self._create("vae_decoder_", self.cfg_c, (batch, h, w), state, dtype, device)

    def decode(self, latents: torch.Tensor, want_rgb8: bool = False):
        """latents f32 [n, latent, h/f, w/f] on the engine's device -> (sample f32 [n, C, h, w], uint8 [n, h, w, C] or None)"""
        n = latents.shape[0]
        if tuple(latents.shape[1:]) != (self.latent_channels, self.h // self.down, self.w // self.down):
            raise SmiError(f"latents {tuple(latents.shape)} do not match the engine's {self.h}x{self.w} image")
        latents = latents.to(torch.float32).contiguous()
        out = torch.empty((n, self.out_channels, self.h, self.w), dtype=torch.float32, device=latents.device)
        rgb = (torch.empty((n, self.h, self.w, self.out_channels), dtype=torch.uint8, device=latents.device)
               if want_rgb8 else None)
        check(lib().smi_vae_decode(self.handle, n, ptr(latents), ptr(out), ptr(rgb)), "smi_vae_decode")
        return out, rgb


class ClipEngine(_EngineBase):
    """CLIP text encoder on the HIP engine (smi_clip_*): token ids -> last hidden state, hidden_states[-2], pooled."""

    def __init__(self, cfg, dtype: torch.dtype, state: dict, batch: int, device):
        self.cfg_c, self.batch, self.dtype = clip_config_c(cfg, dtype), batch, dtype
        self._create("clip_", self.cfg_c, (batch,), state, dtype, device)

    def encode(self, ids: torch.Tensor, eos_pos: torch.Tensor):
        n, L = ids.shape
        if L != self.cfg_c.max_positions:  # the engine always runs max_positions tokens per prompt (smi_clip_encode)
            raise SmiError(f"CLIP text encoder: token ids must be padded to {self.cfg_c.max_positions} positions "
                           f"(padding='max_length'), got {L}")
        dev = self.workspace.device
        d = self.cfg_c.hidden_size
        last = torch.empty((n, L, d), dtype=self.dtype, device=dev)
        pen = torch.empty((n, L, d), dtype=self.dtype, device=dev)
        pooled = torch.empty((n, self.cfg_c.projection_dim or d), dtype=self.dtype, device=dev)
        ids = ids.to(dev, torch.int32).contiguous()
        eos = eos_pos.to(dev, torch.int32).contiguous()
        check(lib().smi_clip_encode(self.handle, n, ptr(ids), ptr(eos), ptr(last), ptr(pen), ptr(pooled)),
              "smi_clip_encode")
        return last, pen, pooled

    def last_layer_out(self, ids: torch.Tensor) -> torch.Tensor:
        """hidden_states[-1]: the last layer's output without the final norm (smi_clip_encode_layers), [n, L, hidden]."""
        n, L = ids.shape
        dev = self.workspace.device
        out = torch.empty((n, L, self.cfg_c.hidden_size), dtype=self.dtype, device=dev)
        ids = ids.to(dev, torch.int32).contiguous()
        check(lib().smi_clip_encode_layers(self.handle, n, ptr(ids), None, None, None, None, ptr(out)), "smi_clip_encode_layers")
        return out


def t5_config_c(cfg, dtype: torch.dtype, max_tokens: int) -> T5ConfigC:
    """cfg: sliders_conceptmod_amd.t5.T5Config (transformers' T5Config values).  A dtype the binding has no code for, and a
    feed-forward other than the gated GELU, are refused here by name; everything else by the library."""
    if dtype not in DTYPE_CODE:
        raise SmiError(f"the T5 encoder runs in bfloat16, got {dtype}")
    if cfg.feed_forward_proj != "gated-gelu":
        raise SmiError(f"T5 feed_forward_proj '{cfg.feed_forward_proj}' is not built: only the gated tanh-GELU "
                       f"(gated-gelu: wi_0 / wi_1) of t5-v1.1 is")
    c = T5ConfigC()
    c.dtype = DTYPE_CODE[dtype]
    c.vocab_size, c.d_model, c.d_kv, c.num_heads = cfg.vocab_size, cfg.d_model, cfg.d_kv, cfg.num_heads
    c.d_ff, c.num_layers = cfg.d_ff, cfg.num_layers
    c.rel_buckets, c.rel_max_distance = cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance
    c.max_tokens, c.eps = max_tokens, cfg.layer_norm_epsilon
    return c


def t5_workspace_bytes(cfg, dtype: torch.dtype, batch: int, max_tokens: int) -> int:
    """smi_t5_workspace_bytes: a host-only dry run (no GPU needed); raises SmiError on a refused config."""
    out = C.c_size_t(0)
    check(lib().smi_t5_workspace_bytes(C.byref(t5_config_c(cfg, dtype, max_tokens)), batch, C.byref(out)),
          "smi_t5_workspace_bytes")
    return out.value


def t5_relative_buckets(num_buckets: int, max_distance: int, L: int) -> List[int]:
    """smi_t5_relative_buckets (host code): the bucket of every offset key - query = -(L - 1) .. L - 1."""
    out = (C.c_int32 * max(2 * L - 1, 1))()
    check(lib().smi_t5_relative_buckets(num_buckets, max_distance, L, out), "smi_t5_relative_buckets")
    return list(out)


class T5Engine(_EngineBase):
    """T5 encoder on the HIP engine (smi_t5_*): token ids [n, L], any 1 <= L <= max_tokens -> last hidden state."""

    def __init__(self, cfg, dtype: torch.dtype, state: dict, batch: int, max_tokens: int, device):
        self.cfg_c, self.batch, self.dtype, self.max_tokens = t5_config_c(cfg, dtype, max_tokens), batch, dtype, max_tokens
        self._create("t5_", self.cfg_c, (batch,), state, dtype, device)

    def encode(self, ids: torch.Tensor) -> torch.Tensor:
        n, L = ids.shape
        dev = self.workspace.device
        out = torch.empty((n, L, self.cfg_c.d_model), dtype=self.dtype, device=dev)
        ids = ids.to(dev, torch.int32).contiguous()
        check(lib().smi_t5_encode(self.handle, n, L, ptr(ids), ptr(out)), "smi_t5_encode")
        return out


def t5_lora_workspace_bytes(cfg, dtype: torch.dtype, sites: Sequence[dict], batch: int, max_tokens: int) -> int:
    """smi_t5_lora_workspace_bytes: a host-only dry run (no GPU needed); raises SmiError on refused sites or shapes."""
    arr, _keep = make_sites(sites)
    out = C.c_size_t(0)
    check(lib().smi_t5_lora_workspace_bytes(C.byref(t5_config_c(cfg, dtype, max_tokens)), arr, len(sites), batch,
                                            C.byref(out)), "smi_t5_lora_workspace_bytes")
    return out.value


class T5LoraEngine(T5Engine):
    """T5 encoder with LoRA sites on its SelfAttention.{q,k,v,o} (smi_t5_lora_*): `encode` as T5Engine, plus a forward with
    one adaptor multiplier per sample that can be saved, and its backward to the flat LoRA gradients."""

    def __init__(self, cfg, dtype: torch.dtype, state: dict, sites: Sequence[dict], batch: int, max_tokens: int, device):
        self.cfg_c, self.batch, self.dtype, self.max_tokens = t5_config_c(cfg, dtype, max_tokens), batch, dtype, max_tokens
        arr, self._site_keep = make_sites(sites)
        out = C.c_size_t(0)
        check(lib().smi_t5_lora_workspace_bytes(C.byref(self.cfg_c), arr, len(sites), batch, C.byref(out)),
              "smi_t5_lora_workspace_bytes")
        self.workspace = torch.empty(out.value, dtype=torch.uint8, device=device)
        warr, self._keep = _weight_table(state, dtype, self.workspace.device)
        handle = C.c_void_p()
        with torch.cuda.device(self.workspace.device):
            check(lib().smi_t5_lora_create(C.byref(self.cfg_c), warr, len(state), arr, len(sites), batch,
                                           ptr(self.workspace), out.value, stream_ptr(), C.byref(handle)),
                  "smi_t5_lora_create")
        self.handle = handle

    def forward_lora(self, ids: torch.Tensor, lora_down: torch.Tensor, lora_up: torch.Tensor, multipliers: Sequence[float],
                     save: bool = False, want=("last_hidden", "penultimate")) -> dict:
        """smi_t5_forward_lora: sample i under the adaptor at multipliers[i].  Returns the outputs named in `want` (model
        dtype): last_hidden = hidden_states[-1] (after the final norm), penultimate = hidden_states[-2]; save=True keeps the
        pass for one `backward`."""
        n, L = ids.shape
        if len(multipliers) != n:
            raise SmiError(f"forward_lora: {len(multipliers)} multipliers for {n} samples")
        dev, d = self.workspace.device, self.cfg_c.d_model
        out = {k: torch.empty((n, L, d), dtype=self.dtype, device=dev) for k in want}
        ids = ids.to(dev, torch.int32).contiguous()
        marr = (C.c_float * n)(*[float(m) for m in multipliers])
        check(lib().smi_t5_forward_lora(self.handle, n, L, ptr(ids), ptr(lora_down), ptr(lora_up), marr, int(save),
                                        ptr(out.get("last_hidden")), ptr(out.get("penultimate"))), "smi_t5_forward_lora")
        return out

    def backward(self, d_hidden: torch.Tensor, d_down: torch.Tensor, d_up: torch.Tensor, which: int = 0):
        """smi_t5_backward: d_hidden fp32 [n, L, d_model], the gradient of last_hidden (which 0) or penultimate (1);
        accumulates (+=) into the flat fp32 gradient buffers."""
        if d_hidden.dtype != torch.float32 or not d_hidden.is_contiguous():
            raise SmiError("backward: d_hidden must be contiguous fp32")
        check(lib().smi_t5_backward(self.handle, int(which), ptr(d_hidden), ptr(d_down), ptr(d_up)), "smi_t5_backward")


def clip_lora_workspace_bytes(cfg, dtype: torch.dtype, sites: Sequence[dict], batch: int) -> int:
    """smi_clip_lora_workspace_bytes: a host-only dry run (no GPU needed); raises SmiError on refused sites or shapes."""
    arr, _keep = make_sites(sites)
    out = C.c_size_t(0)
    check(lib().smi_clip_lora_workspace_bytes(C.byref(clip_config_c(cfg, dtype)), arr, len(sites), batch, C.byref(out)),
          "smi_clip_lora_workspace_bytes")
    return out.value


class ClipLoraEngine(ClipEngine):
    """CLIP text encoder with LoRA sites on its attention projections (smi_clip_lora_*): `encode` as ClipEngine, plus a
    forward with one adaptor multiplier per sample that can be saved, and its backward to the flat LoRA gradients."""

    def __init__(self, cfg, dtype: torch.dtype, state: dict, sites: Sequence[dict], batch: int, device):
        self.cfg_c, self.batch, self.dtype = clip_config_c(cfg, dtype), batch, dtype
        arr, self._site_keep = make_sites(sites)
        out = C.c_size_t(0)
        check(lib().smi_clip_lora_workspace_bytes(C.byref(self.cfg_c), arr, len(sites), batch, C.byref(out)),
              "smi_clip_lora_workspace_bytes")
        self.workspace = torch.empty(out.value, dtype=torch.uint8, device=device)
        warr, self._keep = _weight_table(state, dtype, self.workspace.device)
        handle = C.c_void_p()
        with torch.cuda.device(self.workspace.device):
            check(lib().smi_clip_lora_create(C.byref(self.cfg_c), warr, len(state), arr, len(sites), batch,
                                             ptr(self.workspace), out.value, stream_ptr(), C.byref(handle)),
                  "smi_clip_lora_create")
        self.handle = handle

    def forward_lora(self, ids: torch.Tensor, eos_pos: Optional[torch.Tensor], lora_down: torch.Tensor,
                     lora_up: torch.Tensor, multipliers: Sequence[float], save: bool = False,
                     want=("last_layer_out", "penultimate", "last_hidden", "pooled")) -> dict:
        """smi_clip_forward_lora: sample i under the adaptor at multipliers[i].  Returns the outputs named in `want`
        (model dtype); save=True keeps the pass for one `backward`."""
        n, L = ids.shape
        if L != self.cfg_c.max_positions:
            raise SmiError(f"CLIP text encoder: token ids must be padded to {self.cfg_c.max_positions} positions, got {L}")
        if len(multipliers) != n:
            raise SmiError(f"forward_lora: {len(multipliers)} multipliers for {n} samples")
        dev, d = self.workspace.device, self.cfg_c.hidden_size
        out = {k: torch.empty((n, self.cfg_c.projection_dim or d) if k == "pooled" else (n, L, d), dtype=self.dtype,
                              device=dev) for k in want}
        ids = ids.to(dev, torch.int32).contiguous()
        eos = None if eos_pos is None else eos_pos.to(dev, torch.int32).contiguous()
        marr = (C.c_float * n)(*[float(m) for m in multipliers])
        check(lib().smi_clip_forward_lora(self.handle, n, ptr(ids), ptr(eos), ptr(lora_down), ptr(lora_up), marr, int(save),
                                          ptr(out.get("last_layer_out")), ptr(out.get("penultimate")),
                                          ptr(out.get("last_hidden")), ptr(out.get("pooled"))), "smi_clip_forward_lora")
        return out

    def backward(self, d_hidden: torch.Tensor, d_down: torch.Tensor, d_up: torch.Tensor, which: int = 0):
        """smi_clip_backward: d_hidden fp32 [n, L, hidden], the gradient of last_layer_out (which 0) or penultimate (1);
        accumulates (+=) into the flat fp32 gradient buffers."""
        if d_hidden.dtype != torch.float32 or not d_hidden.is_contiguous():
            raise SmiError("backward: d_hidden must be contiguous fp32")
        check(lib().smi_clip_backward(self.handle, int(which), ptr(d_hidden), ptr(d_down), ptr(d_up)), "smi_clip_backward")


def clip_vision_config_c(cfg, dtype: torch.dtype) -> ClipVisionConfigC:
    """cfg: sliders_conceptmod_amd.clip.CLIPVisionConfig (the transformers config values + the processor's mean / std)."""
    if cfg.hidden_act not in CLIP_ACT:
        raise SmiError(f"CLIP hidden_act '{cfg.hidden_act}' is not built (quick_gelu / gelu)")
    c = ClipVisionConfigC()
    c.dtype = DTYPE_CODE[dtype]
    c.hidden_size, c.num_layers, c.num_heads = cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads
    c.intermediate_size, c.image_size, c.patch_size = cfg.intermediate_size, cfg.image_size, cfg.patch_size
    c.hidden_act, c.projection_dim = CLIP_ACT[cfg.hidden_act], cfg.projection_dim or 0
    for k in range(3):
        c.image_mean[k], c.image_std[k] = float(cfg.image_mean[k]), float(cfg.image_std[k])
    return c


def clip_vision_workspace_bytes(cfg, dtype: torch.dtype, batch: int) -> int:
    """smi_clip_vision_workspace_bytes: a host-only dry run (no GPU needed); raises SmiError on a refused config."""
    out = C.c_size_t(0)
    check(lib().smi_clip_vision_workspace_bytes(C.byref(clip_vision_config_c(cfg, dtype)), batch, C.byref(out)),
          "smi_clip_vision_workspace_bytes")
    return out.value


class ClipVisionEngine(_EngineBase):
    """CLIP image tower on the HIP engine (smi_clip_vision_*): uint8 or normalised float images -> the encoder's output
    and the (projected) class-token embedding."""

    def __init__(self, cfg, dtype: torch.dtype, state: dict, batch: int, device):
        self.cfg_c, self.batch, self.dtype = clip_vision_config_c(cfg, dtype), batch, dtype
        self._create("clip_vision_", self.cfg_c, (batch,), state, dtype, device)

    def encode(self, rgb8: Optional[torch.Tensor] = None, pixel_values: Optional[torch.Tensor] = None,
               want_last_hidden: bool = True):
        """exactly one of rgb8 uint8 [n, S, S, 3] / pixel_values [n, 3, S, S] -> (last_hidden or None, image_embeds)"""
        if (rgb8 is None) == (pixel_values is None):
            raise SmiError("CLIP image tower: pass exactly one of rgb8 / pixel_values")
        c, dev = self.cfg_c, self.workspace.device
        S, G = c.image_size, c.image_size // c.patch_size
        if rgb8 is not None:
            if rgb8.dtype != torch.uint8 or tuple(rgb8.shape[1:]) != (S, S, 3):
                raise SmiError(f"CLIP image tower: rgb8 must be uint8 [n, {S}, {S}, 3], got {rgb8.dtype} "
                               f"{tuple(rgb8.shape)}")
            rgb8 = rgb8.to(dev).contiguous()
            n = rgb8.shape[0]
        else:
            if tuple(pixel_values.shape[1:]) != (3, S, S):
                raise SmiError(f"CLIP image tower: pixel_values must be [n, 3, {S}, {S}], got "
                               f"{tuple(pixel_values.shape)}")
            pixel_values = pixel_values.to(dev, torch.float32).contiguous()
            n = pixel_values.shape[0]
        last = torch.empty((n, G * G + 1, c.hidden_size), dtype=self.dtype, device=dev) if want_last_hidden else None
        emb = torch.empty((n, c.projection_dim or c.hidden_size), dtype=self.dtype, device=dev)
        with torch.cuda.device(dev):
            check(lib().smi_clip_vision_encode(self.handle, n, ptr(rgb8), ptr(pixel_values), ptr(last), ptr(emb)),
                  "smi_clip_vision_encode")
        return last, emb


def clip_logits(image_embeds: torch.Tensor, text_embeds: torch.Tensor, logit_scale: float) -> torch.Tensor:
    """smi_clip_logits: logits_per_image f32 [ni, nt] = exp(logit_scale) <i, t> / (|i| |t|) of 16-bit embeddings."""
    if image_embeds.dtype not in DTYPE_CODE or text_embeds.dtype != image_embeds.dtype:
        raise SmiError(f"clip_logits: embeddings must share float16 / bfloat16, got {image_embeds.dtype} and "
                       f"{text_embeds.dtype}")
    if image_embeds.device.type != "cuda" or text_embeds.device != image_embeds.device:
        raise SmiError("clip_logits: both embeddings must be on the same cuda device (there is no CPU fallback)")
    if image_embeds.ndim != 2 or text_embeds.ndim != 2 or image_embeds.shape[1] != text_embeds.shape[1]:
        raise SmiError(f"clip_logits: shapes {tuple(image_embeds.shape)} and {tuple(text_embeds.shape)} do not match")
    a, b = image_embeds.contiguous(), text_embeds.contiguous()
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        check(lib().smi_clip_logits(DTYPE_CODE[a.dtype], ptr(a), a.shape[0], ptr(b), b.shape[0], a.shape[1],
                                    float(logit_scale), ptr(out), stream_ptr()), "smi_clip_logits")
    return out


def lpips_config_c(channels: Sequence[int], dtype: torch.dtype) -> LpipsConfigC:
    if len(channels) != 5:
        raise SmiError(f"LPIPS: five channel widths expected, got {tuple(channels)}")
    c = LpipsConfigC()
    c.dtype = DTYPE_CODE[dtype]
    for i, v in enumerate(channels):
        c.channels[i] = int(v)
    return c


def lpips_workspace_bytes(channels: Sequence[int], dtype: torch.dtype, max_pairs: int, h: int, w: int) -> int:
    """smi_lpips_workspace_bytes: a host-only dry run (no GPU needed); raises SmiError on a refused config or size."""
    out = C.c_size_t(0)
    check(lib().smi_lpips_workspace_bytes(C.byref(lpips_config_c(channels, dtype)), max_pairs, h, w, C.byref(out)),
          "smi_lpips_workspace_bytes")
    return out.value


def lpips_map_sizes(h: int, w: int):
    """(Ho, Wo) of the five AlexNet taps for an h x w image: conv 11 / 4 / 2, pool 3 / 2, conv 5 / 1 / 2, pool 3 / 2, then 3 / 1 / 1."""
    conv = lambda s, k, st, p: (s + 2 * p - k) // st + 1
    pool = lambda s: (s - 3) // 2 + 1
    h0, w0 = conv(h, 11, 4, 2), conv(w, 11, 4, 2)
    h1, w1 = pool(h0), pool(w0)
    h2, w2 = pool(h1), pool(w1)
    return [(h0, w0), (h1, w1), (h2, w2), (h2, w2), (h2, w2)]


class LpipsEngine(_EngineBase):
    """LPIPS (AlexNet) on the HIP engine for one image size (smi_lpips_*): image pairs -> distances."""

    def __init__(self, channels: Sequence[int], dtype: torch.dtype, state: dict, batch: int, h: int, w: int, device):
        self.channels, self.batch, self.h, self.w, self.dtype = tuple(channels), batch, h, w, dtype
        self.cfg_c = lpips_config_c(channels, dtype)
        self._create("lpips_", self.cfg_c, (batch, h, w), state, dtype, device)

    def distance(self, rgb8_a=None, rgb8_b=None, img_a=None, img_b=None, want_per_layer: bool = False,
                 want_feats: bool = False):
        """exactly one form: uint8 [n, h, w, 3] pairs or f32 [n, 3, h, w] pairs in [-1, 1] -> (dist f32 [n], per_layer
        f32 [n, 5] or None, five post-ReLU taps [2n, Ho, Wo, C] or None)"""
        dev = self.workspace.device
        if (rgb8_a is None) != (rgb8_b is None) or (img_a is None) != (img_b is None) or (rgb8_a is None) == (img_a is None):
            raise SmiError("LPIPS: pass exactly one form, (rgb8_a, rgb8_b) or (img_a, img_b)")
        if rgb8_a is not None:
            want, a, b = (self.h, self.w, 3), rgb8_a, rgb8_b
            if a.dtype != torch.uint8 or b.dtype != torch.uint8:
                raise SmiError(f"LPIPS: rgb8 batches must be uint8, got {a.dtype} and {b.dtype}")
            a, b = a.to(dev).contiguous(), b.to(dev).contiguous()
        else:
            want, a, b = (3, self.h, self.w), img_a, img_b
            a, b = a.to(dev, torch.float32).contiguous(), b.to(dev, torch.float32).contiguous()
        if a.shape != b.shape or a.ndim != 4 or tuple(a.shape[1:]) != want:
            raise SmiError(f"LPIPS: both batches must be [n, {want[0]}, {want[1]}, {want[2]}], got {tuple(a.shape)} and "
                           f"{tuple(b.shape)}")
        n = a.shape[0]
        dist = torch.empty(n, dtype=torch.float32, device=dev)
        per = torch.empty((n, 5), dtype=torch.float32, device=dev) if want_per_layer else None
        feats, fptr = None, None
        if want_feats:
            feats = [torch.empty((2 * n, ho, wo, c), dtype=self.dtype, device=dev)
                     for (ho, wo), c in zip(lpips_map_sizes(self.h, self.w), self.channels)]
            fptr = (C.c_void_p * 5)(*[f.data_ptr() for f in feats])
        u8 = rgb8_a is not None
        with torch.cuda.device(dev):
            check(lib().smi_lpips_distance(self.handle, n, ptr(a) if u8 else None, ptr(b) if u8 else None,
                                           None if u8 else ptr(a), None if u8 else ptr(b), ptr(dist), ptr(per), fptr),
                  "smi_lpips_distance")
        return dist, per, feats
