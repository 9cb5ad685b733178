"""ctypes binding of libplbert_hip.so — the C ABI declared in include/plbert.h.

There is no CPU fallback: if the library is missing or fails to load, every entry point of the
product path raises.  torch is imported first so the library resolves HIP against the same
libamdhip64 torch already mapped (one HIP runtime per process; torch's stream handles are then
valid in our launches).
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL: see module docstring)

HERE = os.path.dirname(os.path.abspath(__file__))
# PLBERT_HIP_LIB: load another build of the same C ABI (kernel timing experiments, tools/build_variant.py)
LIB_PATH = os.environ.get("PLBERT_HIP_LIB") or os.path.join(HERE, "libplbert_hip.so")

PLB_PARAM_NAMES = [
    "encoder.embeddings.word_embeddings.weight",
    "encoder.embeddings.position_embeddings.weight",
    "encoder.embeddings.token_type_embeddings.weight",
    "encoder.embeddings.LayerNorm.weight",
    "encoder.embeddings.LayerNorm.bias",
    "encoder.encoder.embedding_hidden_mapping_in.weight",
    "encoder.encoder.embedding_hidden_mapping_in.bias",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.full_layer_layer_norm.weight",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.full_layer_layer_norm.bias",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.query.weight",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.key.weight",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.value.weight",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.query.bias",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.key.bias",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.value.bias",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.dense.weight",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.dense.bias",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.LayerNorm.weight",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.LayerNorm.bias",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.ffn.weight",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.ffn.bias",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.ffn_output.weight",
    "encoder.encoder.albert_layer_groups.0.albert_layers.0.ffn_output.bias",
    "phoneme_predictor.weight",
    "phoneme_predictor.bias",
    "encoder.pooler.weight",
    "encoder.pooler.bias",
    "token_predictor.weight",
    "token_predictor.bias",
]
PLB_NPARAM = len(PLB_PARAM_NAMES)


class PlbConfig(C.Structure):
    _fields_ = [
        ("vocab_size", C.c_int32), ("embedding_size", C.c_int32), ("hidden_size", C.c_int32),
        ("num_attention_heads", C.c_int32), ("intermediate_size", C.c_int32), ("num_hidden_layers", C.c_int32),
        ("max_position_embeddings", C.c_int32), ("type_vocab_size", C.c_int32), ("layer_norm_eps", C.c_float),
        ("num_phonemes", C.c_int32), ("num_tokens", C.c_int32), ("max_batch", C.c_int32), ("max_seq", C.c_int32),
        ("inference_only", C.c_int32),
    ]


# ---- internal launch structs (csrc/plbert_kernels.h) — used by the kernel-level GPU tests ------------
class PlbGemmNT(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("lda", C.c_int), ("B", C.c_void_p), ("ldb", C.c_int),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("Mstore", C.c_int),
        ("bias", C.c_void_p), ("res", C.c_void_p), ("ldr", C.c_int), ("aux", C.c_void_p), ("ldaux", C.c_int),
        ("C", C.c_void_p), ("ldc", C.c_int), ("C2", C.c_void_p), ("ldc2", C.c_int), ("Cf", C.c_void_p), ("ldcf", C.c_int),
        ("colpart", C.c_void_p),
        ("ce_cols", C.c_int), ("ce_tgt", C.c_void_p), ("ce_pmax", C.c_void_p), ("ce_psum", C.c_void_p),
        ("ce_tlogit", C.c_void_p), ("ce_lse", C.c_void_p), ("ce_w", C.c_void_p),
        ("deq_a", C.c_void_p), ("deq_b", C.c_void_p), ("C8", C.c_void_p), ("ldc8", C.c_int), ("q_scale", C.c_void_p),
        ("q_amax", C.c_void_p), ("c8_bf8", C.c_int),
        ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_mean", C.c_void_p), ("ln_rstd", C.c_void_p),
        ("ln_eps", C.c_float), ("ln_xchg", C.c_void_p), ("ln_err", C.c_void_p), ("ln_fault", C.c_int),
    ]


class PlbGemmTN(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("lda", C.c_int), ("Ncols", C.c_int), ("B", C.c_void_p), ("ldb", C.c_int),
        ("Mtot", C.c_int), ("N", C.c_int), ("K", C.c_int), ("rows_per_split", C.c_int), ("splits", C.c_int),
        ("slab", C.c_void_p), ("deq_a", C.c_void_p), ("deq_b", C.c_void_p),
    ]


class PlbAttn(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("ldqkv", C.c_int), ("lengths", C.c_void_p),
        ("B", C.c_int), ("S", C.c_int), ("NH", C.c_int), ("H", C.c_int), ("scale", C.c_float),
        ("ctx", C.c_void_p), ("ldctx", C.c_int), ("lse", C.c_void_p),
        ("dctx", C.c_void_p), ("lddctx", C.c_int), ("delta", C.c_void_p), ("dqkv", C.c_void_p), ("lddqkv", C.c_int),
        ("colpart", C.c_void_p), ("colpart_accumulate", C.c_int),
        ("ctx8", C.c_void_p), ("ldctx8", C.c_int), ("ctx_scale", C.c_void_p), ("ctx_amax", C.c_void_p),
        ("dqkv8", C.c_void_p), ("lddqkv8", C.c_int), ("dqkv_scale", C.c_void_p), ("dqkv_amax", C.c_void_p),
        ("qoff", C.c_void_p), ("q", C.c_void_p), ("ldq", C.c_int), ("nq_total", C.c_int), ("dq", C.c_void_p), ("lddq", C.c_int),
        ("dq8", C.c_void_p), ("lddq8", C.c_int),
        ("row_start", C.c_void_p),
        ("key_words", C.c_void_p), ("ldkw", C.c_int),
    ]


class PlbEmbed(C.Structure):
    _fields_ = [
        ("ids", C.c_void_p), ("T", C.c_int), ("S", C.c_int), ("E", C.c_int), ("V", C.c_int),
        ("word", C.c_void_p), ("pos", C.c_void_p), ("type0", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("eps", C.c_float), ("out", C.c_void_p), ("ldo", C.c_int), ("dout", C.c_void_p), ("lddo", C.c_int),
        ("dx", C.c_void_p), ("dword", C.c_void_p), ("dpos", C.c_void_p), ("partials", C.c_void_p), ("nblocks", C.c_int),
        ("row_start", C.c_void_p), ("lengths", C.c_void_p), ("B", C.c_int), ("fill_slots", C.c_int),
    ]


class PlbEmbedIn(C.Structure):
    """csrc/plbert_kernels.h: the embedding launches with per-token sources (base: pointer to a PlbEmbed of the caller)."""
    _fields_ = [
        ("base", C.c_void_p), ("token_type_ids", C.c_void_p), ("position_ids", C.c_void_p), ("inputs_embeds", C.c_void_p),
        ("NTY", C.c_int), ("P", C.c_int), ("dtype_rows", C.c_void_p), ("d_inputs_embeds", C.c_void_p),
        ("chunk_part", C.c_void_p),
    ]


class PlbEmbedInputs(C.Structure):
    """include/plbert.h: what a plb_*_inputs call feeds its embeddings beside the ids (device pointers, each optional)."""
    _fields_ = [("token_type_ids", C.c_void_p), ("position_ids", C.c_void_p), ("inputs_embeds", C.c_void_p)]


class PlbPacking(C.Structure):
    """include/plbert.h: the plan of a token-packed call (row_start: device int32 [B+1])."""
    _fields_ = [("row_start", C.c_void_p), ("rows", C.c_int32), ("used", C.c_int32)]


class PlbAdamWGroup(C.Structure):
    """include/plbert.h: one set of AdamW hyper-parameters (doubles, as torch holds them)."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double)]


class PlbAdamWSegment(C.Structure):
    """include/plbert.h: one live segment of a grouped AdamW step with its pre-rounded scalars (plb_adamw_plan)."""
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("group", C.c_int32), ("step", C.c_int32),
                ("decay", C.c_float), ("omb1", C.c_float), ("b2", C.c_float), ("omb2", C.c_float), ("eps", C.c_float),
                ("step_size", C.c_float), ("bc2_sqrt", C.c_float)]


class PlbLambGroup(C.Structure):
    """include/plbert.h: one set of LAMB hyper-parameters; adapt = 0 turns the trust ratio off for the group's tensors."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("adapt", C.c_int32)]


class PlbLambSegment(C.Structure):
    """include/plbert.h: one live tensor of a LAMB step with its pre-rounded scalars (plb_lamb_plan)."""
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("tensor", C.c_int32), ("group", C.c_int32), ("step", C.c_int32),
                ("adapt", C.c_int32), ("omb1", C.c_float), ("b2", C.c_float), ("omb2", C.c_float), ("eps", C.c_float),
                ("bc2_sqrt", C.c_float), ("inv_bc1", C.c_float), ("weight_decay", C.c_float), ("lr", C.c_float)]


class PlbLayerOutputs(C.Structure):
    """include/plbert.h: per-application outputs of plb_forward_layers / plb_encode_layers — two HOST arrays of device
    pointers (L + 1 hidden-state slots, L attention maps; an entry or a whole array may be NULL)."""
    _fields_ = [("hidden_states", C.c_void_p), ("attentions", C.c_void_p)]


class PlbMaskedReport(C.Structure):
    """include/plbert.h: what plb_masked_report writes (every pointer optional, device memory of the caller)."""
    _fields_ = [
        ("pred", C.c_void_p), ("rank", C.c_void_p), ("nll", C.c_void_p), ("topk_ids", C.c_void_p), ("topk_logprob", C.c_void_p),
        ("logits", C.c_void_p), ("sample_loss", C.c_void_p), ("sample_top1", C.c_void_p), ("sample_topk", C.c_void_p),
        ("totals", C.c_void_p), ("token_totals", C.c_void_p),
    ]


class PlbTokenReport(C.Structure):
    """include/plbert.h: what plb_token_report writes (every pointer optional, device memory of the caller)."""
    _fields_ = [
        ("topk_ids", C.c_void_p), ("topk_logprob", C.c_void_p), ("lse", C.c_void_p), ("target_logprob", C.c_void_p),
        ("target_pos", C.c_void_p), ("logits", C.c_void_p), ("totals", C.c_void_p),
    ]


class PlbLayerNorm(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("ldx", C.c_int), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("eps", C.c_float),
        ("y", C.c_void_p), ("ldy", C.c_int), ("mean", C.c_void_p), ("rstd", C.c_void_p),
        ("T", C.c_int), ("H", C.c_int), ("Tzero", C.c_int),
        ("dy", C.c_void_p), ("lddy", C.c_int), ("dx", C.c_void_p), ("lddx", C.c_int),
        ("partials", C.c_void_p), ("nblocks", C.c_int), ("accumulate", C.c_int),
        ("out8", C.c_void_p), ("ld8", C.c_int), ("q_scale", C.c_void_p), ("q_amax", C.c_void_p),
    ]


class PlbMask(C.Structure):
    _fields_ = [
        ("labels", C.c_void_p), ("lengths", C.c_void_p), ("B", C.c_int), ("S", C.c_int),
        ("seed", C.c_uint64), ("step", C.c_uint32),
        ("word_pred_prob", C.c_float), ("mask_prob", C.c_float), ("replace_prob", C.c_float),
        ("mask_id", C.c_int), ("sep_id", C.c_int),
        ("masked", C.c_void_p), ("counts", C.c_void_p), ("idx_padded", C.c_void_p), ("offsets", C.c_void_p),
        ("flat", C.c_void_p),
    ]


class PlbApplyMask(C.Structure):
    _fields_ = [
        ("ids", C.c_void_p), ("sample_off", C.c_void_p), ("word_off", C.c_void_p), ("word_begin", C.c_void_p),
        ("word_len", C.c_void_p), ("action", C.c_void_p), ("repl", C.c_void_p), ("word_token", C.c_void_p),
        ("sep_token", C.c_int64), ("crop_start", C.c_void_p), ("B", C.c_int), ("S", C.c_int), ("mask_id", C.c_int),
        ("labels", C.c_void_p), ("masked", C.c_void_p), ("tokens", C.c_void_p), ("lengths_out", C.c_void_p),
        ("counts", C.c_void_p), ("idx_padded", C.c_void_p), ("offsets", C.c_void_p), ("flat", C.c_void_p),
    ]


# csrc/plbert_kernels.h: the fixed grid of the partial-sum launches and the floats one of its workgroups owns
PLB_NORM_PARTS = 1024


def norm_chunk(n):
    """plb_norm_chunk: floats per workgroup of a partial-sum launch over n floats (whole passes of 256 threads x float4)."""
    return (n + PLB_NORM_PARTS * 1024 - 1) // (PLB_NORM_PARTS * 1024) * 1024


LAMB_CHAIN = 4 + 6 + 3   # PLB_LAMB_CHAIN: the longest chain of fp32 additions behind one partial sum of LAMB's pass 1


def norm_chain(n):
    """PLB_NORM_CHAIN: the longest chain of fp32 additions behind one partial sum of a launch over n floats."""
    return 4 * (norm_chunk(n) // 1024) + 6 + 3


# ---- the signature tables: name -> (restype, [argtypes]), one entry per prototype of the two headers ----------------------
# int / int32_t -> i32, uint32_t -> u32, int64_t -> i64, uint64_t -> u64, size_t -> sz, float -> f32, double -> f64; a
# pointer to a struct mirrored above -> P(that struct); any other pointer and a stream -> vp, or P(scalar) where the callers
# pass byref / a ctypes array. tests/test_binding_host.py holds both tables and the struct mirrors to the headers.
vp, i32, u32, i64, u64, sz, f32, f64, P = (C.c_void_p, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_size_t, C.c_float,
                                           C.c_double, C.POINTER)
# include/plbert.h (the last ten are the test / tuning hooks documented as such at the end of the header)
PUBLIC = {
    "plb_last_error": (C.c_char_p, []),
    "plb_create": (i32, [P(PlbConfig), P(vp)]),
    "plb_destroy": (None, [vp]),
    "plb_param_layout": (i32, [vp, P(i64), P(i64), P(i64), P(i64)]),
    "plb_workspace_bytes": (i64, [vp]),
    "plb_bind": (i32, [vp, vp, vp, vp, vp, vp, i64]),
    "plb_sync_weights": (i32, [vp, vp]),
    "plb_forward": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "plb_pooler": (i32, [vp, vp, i32, i32, vp, vp]),
    "plb_loss_fwd_bwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "plb_loss_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "plb_loss_fwd_bwd_dual": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "plb_adamw_step": (i32, [vp, f64, f64, f64, f64, f64, i32, f64, vp]),
    "plb_grad_norm_floats": (i64, [vp]),
    "plb_grad_accum_bind": (i32, [vp, vp]),
    "plb_grad_accum_add": (i32, [vp, i32, vp, vp]),
    "plb_grad_norm": (i32, [vp, f64, f64, vp, i32, vp]),
    "plb_adamw_step_clipped": (i32, [vp, f64, f64, f64, f64, f64, i32, f64, vp, vp]),
    "plb_adamw_plan": (i32, [vp, P(PlbAdamWGroup), i32, P(i32), i32, P(PlbAdamWSegment), P(i32)]),
    "plb_adamw_step_groups": (i32, [vp, P(PlbAdamWGroup), i32, P(i32), i32, f64, vp, vp]),
    "plb_grad_norm_groups": (i32, [vp, P(i32), f64, f64, vp, vp]),
    "plb_lamb_floats": (i64, [vp]),
    "plb_lamb_plan": (i32, [vp, P(PlbLambGroup), i32, P(i32), i32, P(PlbLambSegment), P(i32)]),
    "plb_lamb_step": (i32, [vp, P(PlbLambGroup), i32, P(i32), i32, f64, vp, vp, vp]),
    "plb_set_fp8": (i32, [vp, i32, vp]),
    "plb_fp8_state": (i32, [vp, P(i32), P(i32)]),
    "plb_fp8_stats": (i32, [vp, P(f32), P(f32), vp]),
    "plb_token_head_steps": (i32, [vp]),
    "plb_set_token_head_steps": (i32, [vp, i32]),
    "plb_comm_unique_id": (i32, [vp]),
    "plb_comm_init": (i32, [vp, vp, i32, i32]),
    "plb_comm_destroy": (i32, [vp]),
    "plb_comm_info": (i32, [vp, P(i32), P(i32), P(i32)]),
    "plb_status": (i32, [vp, P(i32)]),
    "plb_status_ex": (i32, [vp, P(i32), P(i32)]),
    "plb_poll_status": (i32, [vp, P(i32)]),
    "plb_status_export": (i32, [vp, vp, vp]),
    "plb_status_import": (i32, [vp, vp, vp]),
    "plb_last_application_rows": (i32, [vp, P(i64), P(i64)]),
    "plb_packing_plan": (i32, [vp, i32, i32, vp, P(i32), P(i32)]),
    "plb_forward_packed": (i32, [vp, vp, vp, i32, i32, P(PlbPacking), vp, vp, vp, vp]),
    "plb_loss_fwd_bwd_packed": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, P(PlbPacking), vp, vp]),
    "plb_loss_fwd_packed": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, P(PlbPacking), vp, vp, vp]),
    "plb_last_call_rows": (i32, [vp, P(i64), P(i64)]),
    "plb_set_packed_dual": (i32, [vp, i32]),
    "plb_loss_fwd_bwd_dual_packed": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, P(PlbPacking), vp, vp, vp]),
    "plb_set_packed_fp8": (i32, [vp, i32]),
    "plb_encode": (i32, [vp, vp, vp, i32, i32, P(PlbPacking), vp, vp]),
    "plb_encode_bwd": (i32, [vp, vp, vp, i32, i32, P(PlbPacking), vp, vp]),
    "plb_forward_layers": (i32, [vp, vp, vp, i32, i32, P(PlbPacking), vp, P(PlbLayerOutputs), vp]),
    "plb_encode_layers": (i32, [vp, vp, vp, i32, i32, P(PlbPacking), vp, P(PlbLayerOutputs), vp]),
    "plb_encode_bwd_layers": (i32, [vp, vp, vp, i32, i32, P(PlbPacking), vp, vp, vp]),
    "plb_forward_inputs": (i32, [vp, vp, P(PlbEmbedInputs), vp, i32, i32, P(PlbPacking), vp, P(PlbLayerOutputs), vp]),
    "plb_encode_inputs": (i32, [vp, vp, P(PlbEmbedInputs), vp, i32, i32, P(PlbPacking), vp, P(PlbLayerOutputs), vp]),
    "plb_encode_bwd_inputs": (i32, [vp, vp, P(PlbEmbedInputs), vp, i32, i32, P(PlbPacking), vp, vp, vp, vp]),
    "plb_forward_masked": (i32, [vp, vp, P(PlbEmbedInputs), vp, vp, i32, i32, P(PlbPacking), vp, P(PlbLayerOutputs), vp]),
    "plb_encode_masked": (i32, [vp, vp, P(PlbEmbedInputs), vp, vp, i32, i32, P(PlbPacking), vp, P(PlbLayerOutputs), vp]),
    "plb_encode_bwd_masked": (i32, [vp, vp, P(PlbEmbedInputs), vp, vp, i32, i32, P(PlbPacking), vp, vp, vp, vp]),
    "plb_encode_bwd_pooled": (i32, [vp, vp, P(PlbEmbedInputs), vp, vp, i32, i32, P(PlbPacking), vp, vp, vp, vp, vp]),
    "plb_masked_report": (i32, [vp, vp, i32, i32, P(PlbMaskedReport), vp]),
    "plb_token_report": (i32, [vp, vp, vp, vp, i32, i32, i32, P(PlbPacking), vp, i32, P(PlbTokenReport), vp]),
    "plb_comm_pieces": (i32, [vp, P(i32), P(i64)]),
    "plb_broadcast_params": (i32, [vp, i32, vp]),
    "plb_set_grad_overlap": (i32, [vp, i32]),
    "plb_allreduce_grads": (i32, [vp, vp]),
    "plb_apply_mask": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "plb_mask_batch": (i32, [vp, vp, i32, i32, u64, u32, f32, f32, f32, i32, i32, vp, vp, vp, vp, vp]),
    "plb_profile_enable": (None, [i32]),
    "plb_profile_num_classes": (i32, []),
    "plb_profile_class_name": (C.c_char_p, [i32]),
    "plb_profile_read": (i32, [P(f64), P(i64), P(f64), P(f64)]),
    "plb_debug_skip_piece": (None, [i32]),
    "plb_debug_ln_fault": (None, [i32, i32]),
    "plb_debug_hb_audit": (i32, [vp, i32, i32]),
    "plb_debug_hb_report": (i32, [vp, P(i64), P(i32), vp, i32]),
    "plb_comm_trace": (i32, [vp, i32]),
    "plb_comm_trace_read": (i32, [vp, i32, P(i32), P(i64), P(i64), P(f32), P(f32), P(f32)]),
    "plb_set_gemm_nt_tile": (None, [i32]),
    "plb_set_gemm_nt_prefetch": (None, [i32]),
    "plb_set_attn_bwd_fused": (None, [i32]),
    "plb_set_prune_last": (None, [i32]),
}
PUBLIC_SYMBOLS = list(PUBLIC)
# csrc/plbert_kernels.h: the launchers the kernel-level tests and tools call; it declares five of the public hooks again
INTERNAL = {
    **{name: PUBLIC[name] for name in ("plb_set_gemm_nt_tile", "plb_set_gemm_nt_prefetch", "plb_debug_skip_piece",
                                       "plb_debug_ln_fault", "plb_set_attn_bwd_fused")},
    "plb_prof_begin": (i32, [i32, vp, f64, f64]),
    "plb_prof_end": (None, [i32, vp]),
    "plb_launch_gemm_nt_ln": (i32, [P(PlbGemmNT), i32, vp]),
    "plb_launch_gemm_nt_gelud": (i32, [P(PlbGemmNT), i32, vp]),
    "plb_launch_gemm_nt_fp8": (i32, [P(PlbGemmNT), i32, i32, vp]),
    "plb_launch_gemm_nt_fp8_ln": (i32, [P(PlbGemmNT), i32, i32, vp]),
    "plb_launch_gemm_nt_fp8_gelud": (i32, [P(PlbGemmNT), i32, i32, vp]),
    "plb_gemm_nt_fp8_gelud_tile_rows": (i32, [i32]),
    "plb_ln_fault_take": (i32, []),
    "plb_launch_gemm_nt": (i32, [P(PlbGemmNT), i32, i32, vp]),
    "plb_launch_gemm_nt_big": (i32, [P(PlbGemmNT), i32, i32, i32, vp]),
    "plb_gemm_nt_colpart_rows": (i32, [i32, i32, i32]),
    "plb_gemm_nt_plan": (i32, [i32, i32, i32, i32, i32, i32, i32, vp]),   # (PlbGemmNTPlan*: csrc/gemm_nt_plan.h)
    "plb_gemm_tn_plan": (i32, [i64, i32, i32, i32, i32, vp]),   # (PlbGemmTNPlan*: csrc/gemm_tn_plan.h)
    "plb_launch_gemm_tn": (i32, [P(PlbGemmTN), vp]),
    "plb_launch_gemm_tn_fp8": (i32, [P(PlbGemmTN), vp]),
    "plb_launch_gemm_tn_big": (i32, [P(PlbGemmTN), vp]),
    "plb_launch_reduce_slabs": (i32, [vp, i32, sz, vp, i32, vp]),
    "plb_launch_embed_fwd": (i32, [P(PlbEmbed), vp]),
    "plb_launch_embed_bwd": (i32, [P(PlbEmbed), vp]),
    "plb_launch_embed_scatter": (i32, [P(PlbEmbed), i32, vp]),
    "plb_launch_embed_inputs_fwd": (i32, [P(PlbEmbedIn), vp]),
    "plb_launch_embed_inputs_bwd": (i32, [P(PlbEmbedIn), vp]),
    "plb_launch_embed_inputs_scatter": (i32, [P(PlbEmbedIn), vp]),
    "plb_embed_inputs_part_floats": (sz, [i32, i32, i32, i32]),
    "plb_launch_amax": (i32, [vp, i32, sz, i32, i32, vp, vp]),
    "plb_launch_fp8_scales": (i32, [vp, vp, vp, i32, f32, i32, vp]),
    "plb_launch_fp8_scales2": (i32, [vp, vp, vp, i32, f32, i32, i32, f32, vp, i32, vp]),
    "plb_launch_quantize": (i32, [vp, i32, sz, i32, i32, vp, vp, i32, i32, vp]),
    "plb_launch_quantize_multi": (i32, [i32, vp, vp, vp, vp, vp, vp, vp]),
    "plb_launch_ln_fwd": (i32, [P(PlbLayerNorm), vp]),
    "plb_launch_ln_bwd": (i32, [P(PlbLayerNorm), vp]),
    "plb_launch_colsum": (i32, [vp, i32, sz, i32, i32, vp, i32, i32, vp, i32, vp]),
    "plb_launch_copy_cols": (i32, [vp, i32, i32, i32, i32, vp, vp]),
    "plb_launch_pooler": (i32, [vp, i32, i32, i32, vp, vp, vp, vp]),
    "plb_attn_plan": (i32, [i32, i32, i32, i32, vp]),   # (PlbAttnPlan*: csrc/attn_plan.h)
    "plb_attn_args_check": (i32, [P(PlbAttn), i32]),
    "plb_launch_attn_fwd": (i32, [P(PlbAttn), vp]),
    "plb_launch_attn_bwd": (i32, [P(PlbAttn), vp]),
    "plb_launch_attn_bwd_fused": (i32, [P(PlbAttn), vp]),
    "plb_launch_gather_rows": (i32, [vp, i32, vp, i32, i32, i32, vp, i32, vp]),
    "plb_launch_scatter_rows": (i32, [vp, i32, vp, i32, i32, vp, i32, vp]),
    "plb_launch_ce_prepare": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "plb_launch_ce_prepare_packed": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]),
    "plb_launch_unpack_rows": (i32, [vp, i32, i32, vp, vp, i32, i32, i32, vp, vp]),
    "plb_launch_seed_dy": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    "plb_launch_pooler_bwd": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "plb_launch_seed_dy_first_rows": (i32, [vp, vp, vp, i32, i32, i32, vp, vp]),
    "plb_launch_attn_probs": (i32, [vp, i32, vp, vp, vp, i32, i32, i32, f32, vp, vp]),
    "plb_launch_attn_probs_masked": (i32, [vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp]),
    "plb_launch_key_mask_words": (i32, [vp, vp, i32, i32, vp, i32, vp]),
    "plb_launch_add_row_grad": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    "plb_launch_ce_fwd_bwd": (i32, [vp, i32, i32, vp, vp, i32, i32, vp, vp, i32, vp]),
    "plb_launch_sum_rows": (i32, [vp, i32, vp, vp]),
    "plb_launch_token_ce_combine": (i32, [vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "plb_launch_token_ce_combine_packed": (i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]),
    "plb_launch_pack_token_targets": (i32, [vp, vp, vp, i32, i32, i32, vp, vp]),
    "plb_launch_add_scalar": (i32, [vp, vp, vp, vp]),
    "plb_launch_masked_report_rows": (i32, [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
    "plb_launch_masked_report_samples": (i32, [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
    "plb_launch_token_top1": (i32, [vp, i32, vp, vp, i32, vp, vp, vp]),
    "plb_launch_token_topk": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "plb_token_topk_strips": (i32, [i32, i32, i32]),
    "plb_token_topk_scratch_bytes": (sz, [i32]),
    "plb_launch_token_topk_prepare": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]),
    "plb_launch_mask": (i32, [P(PlbMask), vp]),
    "plb_launch_apply_mask": (i32, [P(PlbApplyMask), vp]),
    "plb_launch_adamw": (i32, [vp, vp, vp, vp, vp, sz, f64, f64, f64, f64, f64, i32, f64, vp, i32, vp]),
    "plb_launch_grad_accum": (i32, [vp, vp, sz, i32, vp, vp]),
    "plb_launch_grad_sumsq": (i32, [vp, sz, vp, vp]),
    "plb_launch_grad_norm_finish": (i32, [vp, i32, f64, f64, vp, vp]),
    "plb_launch_adamw_clipped": (i32, [vp, vp, vp, vp, vp, sz, f64, f64, f64, f64, f64, i32, f64, vp, i32, vp, i32, vp]),
    "plb_launch_adamw_segments": (i32, [vp, vp, vp, vp, vp, sz, P(PlbAdamWSegment), i32, f64, vp, i32, vp, i32, vp]),
    "plb_launch_grad_sumsq_segments": (i32, [vp, sz, P(PlbAdamWSegment), i32, vp, vp]),
    "plb_lamb_workgroups": (i64, [P(PlbLambSegment), i32, sz]),
    "plb_launch_lamb_pass1": (i32, [vp, vp, vp, vp, sz, P(PlbLambSegment), i32, f64, vp, i32, vp, i32, vp, vp]),
    "plb_launch_lamb_finish": (i32, [P(PlbLambSegment), i32, sz, i32, i32, vp, vp, vp, vp, vp]),
    "plb_launch_lamb_pass2": (i32, [vp, vp, vp, vp, sz, P(PlbLambSegment), i32, vp, vp, vp, vp]),
    "plb_launch_step_status": (i32, [vp, vp, vp, vp, vp]),
    "plb_launch_status_export": (i32, [vp, vp, vp]),
    "plb_launch_cast_bf16": (i32, [vp, vp, sz, vp]),
    "plb_launch_transpose_cast": (i32, [vp, i32, i32, vp, i32, vp]),
    "plb_launch_transpose_cast_multi": (i32, [i32, vp, vp, vp, vp, vp, vp]),
    "plb_launch_bf16_to_f32": (i32, [vp, i32, vp, i32, i32, i32, vp]),
}


def declare(L):
    """Set restype / argtypes of every table entry that L exports and return L. A symbol L lacks is skipped on its own: a
    build named by PLBERT_HIP_LIB that predates a feature still loads, with everything it does have fully declared."""
    for name, (restype, argtypes) in {**PUBLIC, **INTERNAL}.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, list(argtypes)
    return L


_lib = None


class HipLibraryMissing(RuntimeError):
    pass


def lib():
    """The loaded library; raises HipLibraryMissing (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            f"{LIB_PATH} is missing: build it with `python -m plbert_amd.build` (needs hipcc, gfx950). "
            "There is no CPU fallback for the PL-BERT hot path.")
    try:
        _lib = declare(C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL))
    except OSError as ex:
        raise HipLibraryMissing(f"cannot load {LIB_PATH}: {ex}") from ex
    return _lib


NT_PLAN_FIELDS = ("rc", "family", "tile", "tile_m", "tile_n", "kloop", "grid", "block", "cls", "colpart_rows", "flops", "bytes")


def gemm_nt_plan(M, N, K, form=0, operands=0, opts=0, tile=0):
    """The launch plan of an NT GEMM as a dict of csrc/gemm_nt_plan.h's PlbGemmNTPlan (ten ints, two doubles): what the
    launcher of that form (0 plain, 1 / 2 gelu, 3 / 4 cross-entropy passes, 5 / 6 LayerNorm, 7 / 8 gelu-derivative stash, 9
    fp32 out) and operand kind (0 bf16, 1 / 2 fp8 with e4m3 / e5m2 A) will do; tools size their buffers by it."""
    import struct
    buf = C.create_string_buffer(struct.calcsize("10i2d"))
    lib().plb_gemm_nt_plan(M, N, K, form, operands, opts, tile, buf)
    return dict(zip(NT_PLAN_FIELDS, struct.unpack("10i2d", buf.raw)))


TN_PLAN_FIELDS = ("rc", "kernel", "splits", "rows_per_split", "direct", "grid_x", "grid_y", "block", "slab_floats", "flops")


def gemm_tn_plan(Mtot, Ncols, N, K, operands=0):
    """The launch plan of a token-major weight-gradient GEMM as a dict of csrc/gemm_tn_plan.h's PlbGemmTNPlan (eight ints, an
    int64, a double): kernel (0 small, 1 pipeline, 2 pipeline fp8), row splits and slab need for operands 0 bf16 / 1 fp8."""
    import struct
    buf = C.create_string_buffer(struct.calcsize("8iqd"))
    lib().plb_gemm_tn_plan(Mtot, Ncols, N, K, operands, buf)
    return dict(zip(TN_PLAN_FIELDS, struct.unpack("8iqd", buf.raw)))


ATTN_PLAN_FIELDS = ("rc", "grid", "block", "km", "bwd_form", "bwd_one_samples", "bwd_one_grid", "colpart_rows", "colpart_sample_rows",
                    "unwritten_rows", "cls_fwd", "cls_bwd_dq", "cls_bwd_dkv", "cls_bwd_one", "stat_floats", "fwd_flops", "fwd_bytes",
                    "bwd_flops", "bwd_bytes")
ATTN_PLAN_FORMAT = "14iq4d"
ATTN_PACKED, ATTN_KEYMASK, ATTN_COMPACT, ATTN_OUT_ROWS, ATTN_OUT_IMAGE = 1, 2, 4, 8, 16   # csrc/attn_plan.h: PlbAttnFlags


def attn_plan(B, S, NH, flags=0):
    """The launch plan of the attention kernels as a dict of csrc/attn_plan.h's PlbAttnPlan (fourteen ints, an int64, four
    doubles): grid, kernel variant, the form of the backward under the policy in force (0 two kernels, 1 the single kernel, 2
    hybrid: the first bwd_one_samples samples to the single kernel), partial rows, statistics floats and profiler credit."""
    import struct
    buf = C.create_string_buffer(struct.calcsize(ATTN_PLAN_FORMAT))
    lib().plb_attn_plan(B, S, NH, flags, buf)
    return dict(zip(ATTN_PLAN_FIELDS, struct.unpack(ATTN_PLAN_FORMAT, buf.raw)))


def profile_enable(on):
    lib().plb_profile_enable(int(bool(on)))


def profile_read():
    """{class name: dict(ms, launches, flops, bytes)} for the launches recorded since the last read."""
    L = lib()
    n = L.plb_profile_num_classes()
    ms, fl, by = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
    cnt = (C.c_int64 * n)()
    check(L.plb_profile_read(ms, cnt, fl, by), "plb_profile_read")
    return {L.plb_profile_class_name(i).decode(): dict(ms=ms[i], launches=int(cnt[i]), flops=fl[i], bytes=by[i])
            for i in range(n) if cnt[i]}


def check(rc, what):
    if rc != 0:
        msg = lib().plb_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed: {msg or 'rc=%d' % rc}")
