"""Host side of the HIP engine: device buffers (torch tensors as containers) + the C-ABI calls.

One ``HipEngine`` = one GPU = one set of flat fp32 parameter / gradient / AdamW-moment buffers laid
out as ``plb_param_layout`` says, plus the zero-filled workspace the native engine carves up.
PyTorch supplies memory, streams and (in ``train.py``) ``torch.distributed``; all arithmetic of the
hot path runs in libplbert_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .init import param_shapes


class HandoffTimeout(RuntimeError):
    """A fused LayerNorm launch's in-launch hand-off timed out (include/plbert.h: plb_status): the step it belongs to is
    invalid. By the time this is raised the engine has skipped that step's optimizer update and has been reset
    (exchange buffer and error word zeroed): the caller may simply run the step again."""


class PackingPlan:
    """Plan of a token-packed call (include/plbert.h: PlbPacking), made on the host from the host's lengths: sample b's
    valid tokens are rows [row_start[b], row_start[b] + lengths[b]) of the call's dense token axis, ``rows`` rows are
    executed instead of B*S. ``packed`` is False when the plan is the padded layout itself (nothing to gain): calls that
    are given such a plan run the padded path. ``to(device)`` uploads the table once; the plan can be reused for every
    call with the same lengths (a captured graph included)."""

    def __init__(self, lengths, S):
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32).reshape(-1))
        self.B, self.S = int(lens.shape[0]), int(S)
        self.lengths = lens
        self.row_start_host = np.zeros(self.B + 1, dtype=np.int32)
        rows, used = C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().plb_packing_plan(lens.ctypes.data, self.B, self.S, self.row_start_host.ctypes.data,
                                               C.byref(rows), C.byref(used)), "plb_packing_plan")
        self.rows, self.used = int(rows.value), int(used.value)
        self.row_start = None   # device int32 [B+1] after to()

    @property
    def packed(self):
        return self.rows < (self.B * self.S + 127) // 128 * 128

    @property
    def valid_tokens(self):
        return int(np.clip(self.lengths, 1, self.S).sum())

    def to(self, device, non_blocking=True, pinned=None, out=None):
        """Upload the row table. ``pinned`` / ``out`` (int32, at least B+1 entries): a caller's own pinned staging
        buffer and device tensor (pipeline.DeviceFeeder keeps one pair per slot), so that nothing is allocated here."""
        n = self.B + 1
        if pinned is not None and out is not None:
            pinned[:n].copy_(torch.from_numpy(self.row_start_host))
            out[:n].copy_(pinned[:n], non_blocking=True)
            self.row_start = out[:n]
            return self
        t = torch.from_numpy(self.row_start_host)
        if non_blocking and torch.cuda.is_available():
            t = t.pin_memory()
        self.row_start = t.to(device, non_blocking=non_blocking)
        self._pinned = t   # keeps the staging buffer alive until the copy has run
        return self

    def c_struct(self, device):
        if self.row_start is None or self.row_start.device != torch.device(device):
            self.to(device)
        return _lib.PlbPacking(self.row_start.data_ptr(), self.rows, self.used)


def packing_plan(lengths, S):
    """Host-only: the PackingPlan of a batch with these per-sample lengths padded to S (plb_packing_plan)."""
    return PackingPlan(lengths, S)


def packed_dual_default():
    """PLBERT_PACKED_DUAL=1: dual-head loss calls follow a packing plan that packs (include/plbert.h: plb_set_packed_dual)
    wherever the switch is left open. Anything else, or unset: off."""
    return os.environ.get("PLBERT_PACKED_DUAL", "0").strip() == "1"


def packed_fp8_default():
    """PLBERT_PACKED_FP8=1: calls in fp8 mode follow a packing plan that packs (include/plbert.h: plb_set_packed_fp8)
    wherever the switch is left open. Anything else, or unset: off."""
    return os.environ.get("PLBERT_PACKED_FP8", "0").strip() == "1"


# ---- the encoder and loss entry points (include/plbert.h): which one a call reaches, and its parameters in order ------------
# A call reaches the NARROWEST rung that carries what the caller gave: the error texts name the rung, and a library named
# by PLBERT_HIP_LIB that predates a rung keeps serving the calls that do not need it.
def encoder_entry(family, layers, inputs, key_mask, d_below=None, want_d_inputs_embeds=False, d_pooled=False):
    """The symbol of ``family`` ("forward", "encode", "encode_bwd") for a call with per-application outputs (``layers``),
    embedding inputs (``inputs``) and a key mask (``key_mask``): given or not. "encode_bwd" takes the inputs and the mask of
    its live encode, and ``d_below`` (a list, or None) / ``want_d_inputs_embeds`` in place of ``layers``. The plain
    "forward" rung is HipEngine.forward's (with a plan: that name + "_packed"); forward_layers starts at the layers rung.
    ``d_pooled`` ("encode_bwd" only): a gradient of pooler_output is given — the widest rung, plb_encode_bwd_pooled."""
    if family == "encode_bwd" and d_pooled:
        return "plb_encode_bwd_pooled"
    if family == "encode_bwd":
        layers, inputs = d_below is not None, inputs or want_d_inputs_embeds
    return "plb_" + family + ("_masked" if key_mask else "_inputs" if inputs else "_layers" if layers else "")


def loss_entry(backward, dual, packed):
    """The symbol of a loss call: with the backward or not, dual-head (token_ids given) or not, with a plan or not."""
    return "plb_loss_fwd" + (("_bwd_dual" if dual else "_bwd") if backward else "") + ("_packed" if packed else "")


_ENC = ("e", "ids", "lengths", "B", "S", "packing")
_ENC_IN = ("e", "ids", "inputs", "lengths", "B", "S", "packing")
_ENC_KM = ("e", "ids", "inputs", "key_mask", "lengths", "B", "S", "packing")
_LOSS = ("e", "masked_ids", "labels", "token_ids", "lengths", "idx_offsets", "idx_flat", "n_masked", "B", "S")
_LOSS1 = tuple(n for n in _LOSS if n != "token_ids")   # the phoneme-only training calls take no token_ids
# symbol -> its parameter names as the header has them (tests/test_entry_table_host.py holds the two together):
# HipEngine._entry passes every argument through c_void_p, so nothing else guards the order
ENTRY_ARGS = {
    "plb_forward": _ENC[:-1] + ("hidden", "phoneme_logits", "token_logits", "stream"),
    "plb_forward_packed": _ENC + ("hidden", "phoneme_logits", "token_logits", "stream"),
    "plb_forward_layers": _ENC + ("hidden", "layers", "stream"),
    "plb_forward_inputs": _ENC_IN + ("hidden", "layers", "stream"),
    "plb_forward_masked": _ENC_KM + ("hidden", "layers", "stream"),
    "plb_encode": _ENC + ("hidden", "stream"),
    "plb_encode_layers": _ENC + ("hidden", "layers", "stream"),
    "plb_encode_inputs": _ENC_IN + ("hidden", "layers", "stream"),
    "plb_encode_masked": _ENC_KM + ("hidden", "layers", "stream"),
    "plb_encode_bwd": _ENC + ("d_hidden", "stream"),
    "plb_encode_bwd_layers": _ENC + ("d_hidden", "d_below", "stream"),
    "plb_encode_bwd_inputs": _ENC_IN + ("d_hidden", "d_below", "d_inputs_embeds", "stream"),
    "plb_encode_bwd_masked": _ENC_KM + ("d_hidden", "d_below", "d_inputs_embeds", "stream"),
    "plb_loss_fwd": _LOSS + ("loss", "loss_parts", "stream"),
    "plb_loss_fwd_packed": _LOSS + ("packing", "loss", "loss_parts", "stream"),
    "plb_loss_fwd_bwd": _LOSS1 + ("loss", "stream"),
    "plb_loss_fwd_bwd_packed": _LOSS1 + ("packing", "loss", "stream"),
    "plb_loss_fwd_bwd_dual": _LOSS + ("loss", "loss_parts", "stream"),
    "plb_loss_fwd_bwd_dual_packed": _LOSS + ("packing", "loss", "loss_parts", "stream"),
}
# the rung only a gradient of pooler_output reaches (tests/test_pooler_bwd_host.py holds it to the header like the table above)
POOLED_ENTRY_ARGS = {
    "plb_encode_bwd_pooled": _ENC_KM + ("d_hidden", "d_below", "d_inputs_embeds", "d_pooled", "stream"),
}


class HipEngine:
    def __init__(self, cfg, num_phonemes, num_tokens=0, max_batch=32, max_seq=512, device=None, train=True):
        """``train=False``: inference / validation engine (README.md:91, train.py:288-304) — no gradient, moment or
        per-layer activation buffers (forward and loss-only calls work, backward and AdamW raise).
        PLBERT_PACKED_DUAL=1 in the environment turns ``set_packed_dual`` on at creation, PLBERT_PACKED_FP8=1
        ``set_packed_fp8``."""
        cfg.check_supported()
        if not torch.cuda.is_available():
            raise RuntimeError("HipEngine needs a ROCm GPU (torch.cuda.is_available() is False); "
                               "the PL-BERT hot path has no CPU fallback")
        self.cfg = cfg
        self.num_phonemes, self.num_tokens = int(num_phonemes), int(num_tokens)
        self.max_batch, self.max_seq = int(max_batch), int(max_seq)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.train_mode = bool(train)
        self.L = _lib.lib()
        c = _lib.PlbConfig(cfg.vocab_size, cfg.embedding_size, cfg.hidden_size, cfg.num_attention_heads,
                           cfg.intermediate_size, cfg.num_hidden_layers, cfg.max_position_embeddings,
                           cfg.type_vocab_size, cfg.layer_norm_eps, self.num_phonemes, self.num_tokens,
                           self.max_batch, self.max_seq, 0 if train else 1)
        h = C.c_void_p()
        _lib.check(self.L.plb_create(C.byref(c), C.byref(h)), "plb_create")
        self.handle = h
        offs = (C.c_int64 * _lib.PLB_NPARAM)()
        sizes = (C.c_int64 * _lib.PLB_NPARAM)()
        total, trainable = C.c_int64(), C.c_int64()
        _lib.check(self.L.plb_param_layout(h, offs, sizes, C.byref(total), C.byref(trainable)), "plb_param_layout")
        self.total, self.trainable = int(total.value), int(trainable.value)
        shapes = param_shapes(cfg, self.num_phonemes, self.num_tokens)
        self.layout = OrderedDict()
        for i, name in enumerate(_lib.PLB_PARAM_NAMES):
            if sizes[i] == 0:
                continue
            shp = shapes[name]
            assert int(np.prod(shp)) == sizes[i], (name, shp, sizes[i])
            self.layout[name] = (int(offs[i]), int(sizes[i]), tuple(shp))
        # every C-ABI call below runs with this engine's device current (plb_bind creates its side stream and events
        # there; launches go to that device's streams): HipEngine(device="cuda:1") works while cuda:0 is current
        with torch.cuda.device(self.device):
            z = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)
            self.params = z(self.total)
            self._loss = z(1)
            self._loss_parts = z(2)
        # gradients, AdamW moments and the workspace are allocated by the first call that computes (_bind): a model
        # that is only constructed, or whose parameters move into another engine (model.py: _adopt), holds its
        # parameters and nothing else
        self._grads = self._exp_avg = self._exp_avg_sq = self.workspace = None
        self.ws_bytes = int(self.L.plb_workspace_bytes(h))
        self._bound = False
        self._synced_version = -1
        self.comm_world = 1
        self._on_handoff_timeout = []   # callbacks(err): owners of an optimizer step count rewind it by err.skipped_updates
        self.packed_dual = False
        if packed_dual_default():
            self.set_packed_dual(True)
        self.packed_fp8 = False
        if packed_fp8_default():
            self.set_packed_fp8(True)

    def _bind(self):
        if self._bound:
            return
        with torch.cuda.device(self.device):
            z = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)
            if self.train_mode:
                self._grads, self._exp_avg, self._exp_avg_sq = z(self.total), z(self.total), z(self.total)
            self.workspace = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=self.device)
            p = lambda t: None if t is None else t.data_ptr()
            # plb_bind creates the engine's side stream and events on the current device
            _lib.check(self.L.plb_bind(self.handle, self.params.data_ptr(), p(self._grads), p(self._exp_avg),
                                       p(self._exp_avg_sq), self.workspace.data_ptr(), self.ws_bytes), "plb_bind")
        self._bound = True

    # flat fp32 gradient / AdamW-moment buffers (None on an inference engine); first access allocates
    @property
    def grads(self):
        if self.train_mode:
            self._bind()
        return self._grads

    @property
    def exp_avg(self):
        if self.train_mode:
            self._bind()
        return self._exp_avg

    @property
    def exp_avg_sq(self):
        if self.train_mode:
            self._bind()
        return self._exp_avg_sq

    def device_bytes(self):
        """Bytes of device memory this engine holds."""
        ts = [self.params, self._grads, self._exp_avg, self._exp_avg_sq, self.workspace,
              getattr(self, "_accum", None), getattr(self, "_norm_buf", None), getattr(self, "_lamb_buf", None)]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.L.plb_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ---- parameters -------------------------------------------------------------------------------------
    def view(self, name, of=None):
        off, n, shp = self.layout[name]
        return (self.params if of is None else of)[off:off + n].view(shp)

    def load_state_dict(self, sd, strict=True):
        """Copy tensors / arrays keyed by reference state-dict names into the flat buffer.
        ``module.`` prefixes are stripped as train.py:98 does."""
        seen = set()
        for k, v in sd.items():
            k = k.replace("module.", "")
            if k not in self.layout:
                if strict and not (k.endswith("position_ids") or k.endswith("token_type_ids")):
                    raise KeyError(f"unexpected key {k}")
                continue
            t = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v)
            self.view(k).copy_(t.to(self.device, torch.float32))
            seen.add(k)
        if strict:
            missing = [k for k in self.layout if k not in seen]
            if missing:
                raise KeyError(f"missing keys {missing}")
        self._synced_version = -1  # the compute copies are refreshed by the next call that computes

    def state_dict(self):
        return OrderedDict((k, self.view(k).detach().clone()) for k in self.layout)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def sync_weights(self):
        """Refresh the bf16 / transposed compute copies from the fp32 parameters. Automatic after load_state_dict,
        AdamW and any in-place op torch tracks on the parameters; call it yourself after writing through ``.data``
        (which bypasses torch's version counter)."""
        self._bind()
        with torch.cuda.device(self.device):
            _lib.check(self.L.plb_sync_weights(self.handle, self._stream()), "plb_sync_weights")
        self._synced_version = self.params._version

    def _ensure_synced(self):
        self._bind()
        if self.params._version != self._synced_version:
            self.sync_weights()

    # ---- data-parallel exchange (plb_comm_*) ------------------------------------------------------------
    def comm_init(self, unique_id: bytes, rank: int, world: int):
        """Attach an RCCL communicator (collective: every rank calls it with rank 0's ``comm_unique_id()``)."""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._bind()
        with torch.cuda.device(self.device):
            _lib.check(self.L.plb_comm_init(self.handle, buf, int(rank), int(world)), "plb_comm_init")
        self.comm_world = int(world)

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _lib.check(_lib.lib().plb_comm_unique_id(buf), "plb_comm_unique_id")
        return bytes(buf)

    def comm_info(self):
        r, w, v = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self.L.plb_comm_info(self.handle, C.byref(r), C.byref(w), C.byref(v)), "plb_comm_info")
        return int(r.value), int(w.value), int(v.value)

    def status(self):
        """{'ln_exchange_timeouts': n} — synchronises the device (plb_status); a non-zero report resets the exchange
        state, so it is reported once."""
        n, k = C.c_int32(), C.c_int32()
        with torch.cuda.device(self.device):
            _lib.check(self.L.plb_status_ex(self.handle, C.byref(n), C.byref(k)), "plb_status_ex")
        return {"ln_exchange_timeouts": int(n.value), "skipped_updates": int(k.value)}

    def poll_status(self):
        """The same count WITHOUT synchronising: as of the last loss call that has completed on the device."""
        if not self._bound:
            return {"ln_exchange_timeouts": 0}
        n = C.c_int32()
        _lib.check(self.L.plb_poll_status(self.handle, C.byref(n)), "plb_poll_status")
        return {"ln_exchange_timeouts": int(n.value)}

    def raise_if_failed(self):
        """Raise HandoffTimeout if a completed step reported a timed-out hand-off. Costs one read of a pinned host
        word: called at the top of every training step (one step late at worst — the device has already left the
        failed step's update out) and wherever a loss has just been read back (exact)."""
        if self.poll_status()["ln_exchange_timeouts"]:
            st = self.status()   # synchronises, reports once and resets the exchange state
            err = HandoffTimeout(f"{st['ln_exchange_timeouts']} in-launch LayerNorm hand-off(s) timed out: the loss of "
                                 f"that step is NaN and {st['skipped_updates']} optimizer update(s) were skipped on the "
                                 "device; the engine has been reset, re-run the step")
            err.skipped_updates = st["skipped_updates"]
            for fn in self._on_handoff_timeout:
                fn(err)
            raise err

    def status_exchange(self, all_reduce):
        """For a host-side gradient exchange (torch.distributed fallback): let the step's health word travel with the
        gradients — export this rank's count, ``all_reduce(tensor)`` sums it over the ranks in place, import merges the
        sum (every rank then skips the update, returns a NaN loss and raises HandoffTimeout, or none does). With the
        engine's own communicator the same happens inside plb_loss_fwd_bwd."""
        if not hasattr(self, "_status_f"):
            self._status_f = torch.zeros(1, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.plb_status_export(self.handle, self._status_f.data_ptr(), self._stream()), "plb_status_export")
            all_reduce(self._status_f)
            _lib.check(self.L.plb_status_import(self.handle, self._status_f.data_ptr(), self._stream()), "plb_status_import")

    def hb_audit(self, on=True, break_wait=-1):
        """Debug: happens-before audit of the backward's streams (include/plbert.h: plb_debug_hb_audit)."""
        _lib.check(self.L.plb_debug_hb_audit(self.handle, int(bool(on)), int(break_wait)), "plb_debug_hb_audit")

    def hb_report(self):
        n, v = C.c_int64(), C.c_int32()
        buf = C.create_string_buffer(512)
        _lib.check(self.L.plb_debug_hb_report(self.handle, C.byref(n), C.byref(v), buf, 512), "plb_debug_hb_report")
        return {"checks": int(n.value), "violations": int(v.value), "first": buf.value.decode()}

    def comm_trace(self, on=True):
        _lib.check(self.L.plb_comm_trace(self.handle, int(bool(on))), "plb_comm_trace")

    def comm_trace_read(self, max_pieces=16):
        """Per piece of the last loss call: (begin, end) float range, release and completion time in ms since the call's
        first launch; plus (begin, end) of the weight-gradient tail. Synchronises on the trace events."""
        n = C.c_int32()
        a, b = (C.c_int64 * max_pieces)(), (C.c_int64 * max_pieces)()
        r, d, t = (C.c_float * max_pieces)(), (C.c_float * max_pieces)(), (C.c_float * 2)()
        with torch.cuda.device(self.device):
            _lib.check(self.L.plb_comm_trace_read(self.handle, max_pieces, C.byref(n), a, b, r, d, t), "plb_comm_trace_read")
        return {"tail_ms": [round(t[0], 4), round(t[1], 4)],
                "pieces": [{"range": [int(a[i]), int(b[i])], "released_ms": round(r[i], 4), "done_ms": round(d[i], 4)}
                           for i in range(n.value)]}

    def last_application_rows(self):
        """(rows, of): token rows the last loss call ran the post-attention part of its last application on, of the
        call's padded token count (plb_last_application_rows)."""
        r, o = C.c_int64(), C.c_int64()
        _lib.check(self.L.plb_last_application_rows(self.handle, C.byref(r), C.byref(o)), "plb_last_application_rows")
        return int(r.value), int(o.value)

    def last_call_rows(self):
        """(rows, of): token rows the last forward / loss call executed and the B*S it stood for (plb_last_call_rows);
        rows < of: the call ran token-packed."""
        r, o = C.c_int64(), C.c_int64()
        _lib.check(self.L.plb_last_call_rows(self.handle, C.byref(r), C.byref(o)), "plb_last_call_rows")
        return int(r.value), int(o.value)

    def set_packed_dual(self, on=True):
        """Dual-head loss calls (``token_ids`` given) that are handed a PackingPlan that packs run token-packed, token head
        included (plb_set_packed_dual). Off (the default): they run padded, plan or not. Host state only."""
        _lib.check(self.L.plb_set_packed_dual(self.handle, int(bool(on))), "plb_set_packed_dual")
        self.packed_dual = bool(on)

    def set_packed_fp8(self, on=True):
        """Calls in fp8 mode (``set_fp8``) that are handed a PackingPlan that packs run token-packed: the calibration
        calls and the fp8 calls alike (plb_set_packed_fp8). Dual-head calls need ``set_packed_dual`` as well. Off (the
        default): every call in fp8 mode runs padded, plan or not. Host state only."""
        _lib.check(self.L.plb_set_packed_fp8(self.handle, int(bool(on))), "plb_set_packed_fp8")
        self.packed_fp8 = bool(on)

    def _packing(self, packing, B, S):
        if packing is None:
            return None
        if packing.B != B or packing.S != S:
            raise ValueError(f"packing plan made for {packing.B} x {packing.S}, the batch is {B} x {S}")
        return packing.c_struct(self.device)

    def comm_pieces(self):
        """(collectives, floats) of the last step's gradient exchange."""
        n, f = C.c_int32(), C.c_int64()
        _lib.check(self.L.plb_comm_pieces(self.handle, C.byref(n), C.byref(f)), "plb_comm_pieces")
        return int(n.value), int(f.value)

    def comm_destroy(self):
        with torch.cuda.device(self.device):
            self.L.plb_comm_destroy(self.handle)
        self.comm_world = 1

    def set_grad_overlap(self, on):
        _lib.check(self.L.plb_set_grad_overlap(self.handle, int(bool(on))), "plb_set_grad_overlap")

    def broadcast_params(self, root=0):
        self._bind()
        with torch.cuda.device(self.device):
            _lib.check(self.L.plb_broadcast_params(self.handle, int(root), self._stream()), "plb_broadcast_params")
        self._synced_version = self.params._version

    def allreduce_grads(self):
        with torch.cuda.device(self.device):
            _lib.check(self.L.plb_allreduce_grads(self.handle, self._stream()), "plb_allreduce_grads")

    def set_fp8(self, on=True):
        """fp8 (e4m3 / e5m2) MFMA path for the QKV / FFN GEMMs (plb_set_fp8); the next call calibrates in bf16."""
        self._bind()
        with torch.cuda.device(self.device):
            _lib.check(self.L.plb_set_fp8(self.handle, int(bool(on)), self._stream()), "plb_set_fp8")

    def fp8_state(self):
        a, b = C.c_int32(), C.c_int32()
        _lib.check(self.L.plb_fp8_state(self.handle, C.byref(a), C.byref(b)), "plb_fp8_state")
        return bool(a.value), bool(b.value)

    FP8_SITES = ("x", "a", "gelu_u", "context", "dpre2", "dU", "dpre1", "dQKV")

    def fp8_stats(self):
        """{site: (calls in which values were clamped, worst overshoot)} since set_fp8 (plb_fp8_stats; synchronises)."""
        c, w = (C.c_float * 8)(), (C.c_float * 8)()
        with torch.cuda.device(self.device):
            _lib.check(self.L.plb_fp8_stats(self.handle, c, w, self._stream()), "plb_fp8_stats")
        return {n: (int(c[i]), round(float(w[i]), 4)) for i, n in enumerate(self.FP8_SITES)}

    @property
    def token_head_steps(self):
        return int(self.L.plb_token_head_steps(self.handle))

    @token_head_steps.setter
    def token_head_steps(self, n):
        _lib.check(self.L.plb_set_token_head_steps(self.handle, int(n)), "plb_set_token_head_steps")

    # ---- calls --------------------------------------------------------------------------------------------
    def _dev_i64(self, x):
        t = torch.as_tensor(x)
        if t.dtype != torch.int64 or t.device != self.device or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.int64, non_blocking=True).contiguous()
        return t

    def _dev_i32(self, x):
        if x is None:
            return None
        t = torch.as_tensor(x)
        if t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous()
        return t

    # ---- embedding inputs (include/plbert.h: PlbEmbedInputs) ----
    def _embed_inputs(self, ids, token_type_ids, position_ids, inputs_embeds):
        """(ids | None, B, S, PlbEmbedInputs | None, the tensors it points to). Exactly one of ``ids`` and
        ``inputs_embeds``; ``position_ids`` [B,S] or [1,S] (broadcast); index ranges are checked here, on the host side of
        the call, with the argument and its bound in the text."""
        if (ids is None) == (inputs_embeds is None):
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
        E = self.cfg.embedding_size
        xe = None
        if ids is not None:
            ids = self._dev_i64(ids)
            B, S = ids.shape
        else:
            xe = torch.as_tensor(inputs_embeds)
            if xe.dim() != 3 or xe.shape[-1] != E:
                raise ValueError(f"inputs_embeds must be [B,S,embedding_size={E}], got {tuple(xe.shape)}")
            xe = xe.detach().to(device=self.device, dtype=torch.float32).contiguous()
            B, S = int(xe.shape[0]), int(xe.shape[1])

        def index(t, what, bound, bound_name):
            if t is None:
                return None
            t = torch.as_tensor(t)
            if what == "position_ids" and t.dim() == 2 and t.shape[0] == 1 and B > 1:
                t = t.expand(B, -1)
            if tuple(t.shape) != (B, S):
                raise ValueError(f"{what} must be [{B},{S}]{' or [1,' + str(S) + ']' if what == 'position_ids' else ''}, got {tuple(t.shape)}")
            t = t.to(device=self.device, dtype=torch.int64).contiguous()
            lo, hi = int(t.min()), int(t.max())
            if lo < 0 or hi >= bound:
                raise ValueError(f"{what} has values in [{lo}, {hi}]: they must be in [0, {bound_name} = {bound})")
            return t

        tt = index(token_type_ids, "token_type_ids", self.cfg.type_vocab_size, "type_vocab_size")
        pid = index(position_ids, "position_ids", self.cfg.max_position_embeddings, "max_position_embeddings")
        if tt is None and pid is None and xe is None:
            return ids, int(B), int(S), None, None
        p = lambda t: None if t is None else t.data_ptr()
        return ids, int(B), int(S), _lib.PlbEmbedInputs(p(tt), p(pid), p(xe)), (tt, pid, xe)

    def _key_mask(self, key_mask, B, S):
        """A key mask (include/plbert.h: plb_*_masked) as the int32 [B,S] device tensor the calls take, or None."""
        if key_mask is None:
            return None
        m = torch.as_tensor(key_mask)
        if tuple(m.shape) != (B, S):
            raise ValueError(f"key_mask must be [{B},{S}], got {tuple(m.shape)}")
        return (m != 0).to(device=self.device, dtype=torch.int32).contiguous()

    def forward(self, ids, lengths=None, want_hidden=False, want_phoneme=True, want_token=False, packing=None,
                token_type_ids=None, position_ids=None, inputs_embeds=None):
        """ids int64 [B,S]; lengths per-sample valid-token counts (None = no padding).
        Returns (hidden | None, phoneme_logits | None, token_logits | None), fp32 on the device.
        ``packing`` (PackingPlan of these lengths): token-packed execution; pad positions of the outputs are zeros.
        With all three ``want_*`` False the call outputs nothing: it runs the encoder and leaves the final hidden state
        on the device for ``token_report``.
        ``token_type_ids`` / ``position_ids`` / ``inputs_embeds`` (plb_forward_inputs; ``ids`` is None with
        ``inputs_embeds``): the hidden state only — pass want_phoneme=False (the logits of such a call are not computed)."""
        self._ensure_synced()
        if token_type_ids is not None or position_ids is not None or inputs_embeds is not None:
            if want_phoneme or want_token:
                raise ValueError("forward: token_type_ids / position_ids / inputs_embeds give the hidden state only "
                                 "(want_phoneme=False, want_token=False)")
            hs, at, hid = self.forward_layers(ids, lengths, packing, hidden_states=False, attentions=False, want_hidden=True,
                                              token_type_ids=token_type_ids, position_ids=position_ids,
                                              inputs_embeds=inputs_embeds)
            return (hid if want_hidden else None), None, None
        ids = self._dev_i64(ids)
        B, S = ids.shape
        lens = self._dev_i32(lengths)
        with torch.cuda.device(self.device):
            hid = torch.empty((B, S, self.cfg.hidden_size), dtype=torch.float32, device=self.device) if want_hidden else None
            ph = torch.empty((B, S, self.num_phonemes), dtype=torch.float32, device=self.device) if want_phoneme else None
            tk = torch.empty((B, S, self.num_tokens), dtype=torch.float32, device=self.device) if want_token else None
            pk = self._packing(packing, B, S)
            self._entry(encoder_entry("forward", False, False, False) + ("" if pk is None else "_packed"),
                        dict(ids=ids, lengths=lens, B=B, S=S, packing=pk, hidden=hid, phoneme_logits=ph, token_logits=tk))
        self._last_encoder_call = (int(B), int(S), lens, packing)
        return hid, ph, tk

    def _entry(self, name, pieces):
        """Call the entry point ``name`` with its ENTRY_ARGS out of ``pieces`` (the handle and the current stream are added
        here): a device tensor goes in as its pointer, a ctypes struct by reference, a ctypes pointer array by address, an
        int as it is and None as NULL."""
        def arg(v):
            if v is None or isinstance(v, (int, C.c_void_p)):
                return v
            if torch.is_tensor(v):
                return v.data_ptr()
            return C.byref(v) if isinstance(v, C.Structure) else C.addressof(v)
        pieces = dict(pieces, e=self.handle, stream=self._stream())
        names = ENTRY_ARGS[name] if name in ENTRY_ARGS else POOLED_ENTRY_ARGS[name]
        _lib.check(getattr(self.L, name)(*[arg(pieces[k]) for k in names]), name)

    # ---- per-application outputs (include/plbert.h: PlbLayerOutputs) ----
    @staticmethod
    def _slot_choice(want, n, what):
        """True -> every slot, False / None -> none, a list -> those slots (negative indices count from the end)."""
        if want is True:
            return list(range(n))
        if not want:
            return []
        idx = sorted({int(i) + n if int(i) < 0 else int(i) for i in want})
        if idx and not (0 <= idx[0] and idx[-1] < n):
            raise ValueError(f"{what}: slot outside [0, {n})")
        return idx

    def _alloc_layer_outputs(self, B, S, hidden_states, attentions):
        """(hidden-state tensors [L+1], attention tensors [L]) with None in the slots not asked for; nothing is zeroed:
        the call writes every element of what it is handed."""
        nl, H, NH = self.cfg.num_hidden_layers, self.cfg.hidden_size, self.cfg.num_attention_heads
        hs, at = [None] * (nl + 1), [None] * nl
        for i in self._slot_choice(hidden_states, nl + 1, "hidden_states"):
            hs[i] = torch.empty((B, S, H), dtype=torch.float32, device=self.device)
        for i in self._slot_choice(attentions, nl, "attentions"):
            at[i] = torch.empty((B, NH, S, S), dtype=torch.float32, device=self.device)
        return hs, at

    def _ptr_array(self, tensors, n, what, shape=None):
        """Host array of n device pointers (None -> NULL) over ``tensors``, or None when there is nothing in it."""
        if tensors is None:
            return None
        tensors = list(tensors)
        if len(tensors) != n:
            raise ValueError(f"{what}: {len(tensors)} entries, the model has {n} slots")
        for t in tensors:
            if t is not None and (t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous()
                                  or (shape is not None and tuple(t.shape) != tuple(shape))):
                raise ValueError(f"{what}: every entry must be a contiguous fp32 tensor{'' if shape is None else ' ' + str(list(shape))} "
                                 f"on {self.device}")
        if all(t is None for t in tensors):
            return None
        return (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in tensors])

    def _layer_outputs(self, hs, at, B, S):
        """(PlbLayerOutputs or None, what must stay alive across the call)"""
        nl, H, NH = self.cfg.num_hidden_layers, self.cfg.hidden_size, self.cfg.num_attention_heads
        ha = self._ptr_array(hs, nl + 1, "hidden_states", (B, S, H))
        aa = self._ptr_array(at, nl, "attentions", (B, NH, S, S))
        if ha is None and aa is None:
            return None, None
        lo = _lib.PlbLayerOutputs(None if ha is None else C.addressof(ha), None if aa is None else C.addressof(aa))
        return lo, (ha, aa)

    def forward_layers(self, ids, lengths=None, packing=None, hidden_states=True, attentions=False, want_hidden=False,
                       out=None, token_type_ids=None, position_ids=None, inputs_embeds=None, key_mask=None):
        """The encoder's per-application outputs (plb_forward_layers): ``hidden_states`` / ``attentions`` = True (every
        slot), False, or a list of slots. Returns ``(hidden_states, attentions)``: lists of L + 1 fp32 [B,S,H] and of L
        fp32 [B,NH,S,S] tensors with None in the slots not asked for; ``hidden_states[0]`` is the output of
        embedding_hidden_mapping_in, ``hidden_states[l]`` the output of application l. Pad positions of every hidden
        state and pad query rows / key columns of every attention map are zeros. ``want_hidden``: a third element, the
        ``hidden`` of ``forward`` itself. ``out`` = (hidden-state list, attention list): the caller's tensors (None = slot
        not wanted) instead of new ones. Works on inference-only engines, with a plan, and in fp8 mode.
        ``token_type_ids`` / ``position_ids`` / ``inputs_embeds`` (plb_forward_inputs, not in fp8 mode): the embedding
        inputs of transformers' AlbertModel; ``ids`` is None with ``inputs_embeds`` [B,S,embedding_size].
        ``key_mask`` [B,S], nonzero = attend (plb_forward_masked, not in fp8 mode): a mask that need not be a prefix;
        ``lengths`` is then each sample's extent, 1 + its last valid position. A masked position below the extent (a hole)
        is removed as a key only: its column of every attention map is zeros, its own row and hidden state are computed."""
        self._ensure_synced()
        ids, B, S, ein, keep_in = self._embed_inputs(ids, token_type_ids, position_ids, inputs_embeds)
        lens = self._dev_i32(lengths)
        km = self._key_mask(key_mask, B, S)
        with torch.cuda.device(self.device):
            hs, at = self._alloc_layer_outputs(B, S, hidden_states, attentions) if out is None else (list(out[0]), list(out[1]))
            hid = torch.empty((B, S, self.cfg.hidden_size), dtype=torch.float32, device=self.device) if want_hidden else None
            lo, keep = self._layer_outputs(hs, at, B, S)
            self._entry(encoder_entry("forward", True, ein is not None, km is not None),
                        dict(ids=ids, inputs=ein, key_mask=km, lengths=lens, B=B, S=S, packing=self._packing(packing, B, S),
                             hidden=hid, layers=lo))
            del keep, keep_in
        self._last_encoder_call = (int(B), int(S), lens, packing)
        return (hs, at, hid) if want_hidden else (hs, at)

    def encode(self, ids, lengths=None, packing=None, layers=None, token_type_ids=None, position_ids=None, inputs_embeds=None,
               key_mask=None):
        """Differentiable forward (include/plbert.h: plb_encode): ``.last_hidden_state`` fp32 [B,S,H] with every
        application's activations kept for ``encode_bwd``; ZEROS at pad positions. Training engines only, not in fp8
        mode. The ids, lengths and plan are remembered for the backward; any other computing call on this engine in
        between (forward, a loss call, another encode, an optimizer step) ends the life of the kept activations.
        ``layers`` = dict(hidden_states=True | False | slots, attentions=...) (plb_encode_layers): returns
        ``(hidden, hidden_states, attentions)`` as ``forward_layers`` does.
        ``token_type_ids`` / ``position_ids`` / ``inputs_embeds`` (plb_encode_inputs): the embedding inputs of
        transformers' AlbertModel, remembered for the backward like the ids; ``ids`` is None with ``inputs_embeds``.
        ``key_mask`` [B,S] (plb_encode_masked): as in ``forward_layers``; remembered for the backward like the ids."""
        if not self.train_mode:
            raise RuntimeError("this HipEngine was built with train=False (inference / validation only): encode() keeps "
                               "the activations of every layer for a backward")
        self.raise_if_failed()
        self._ensure_synced()
        ids, B, S, ein, keep_in = self._embed_inputs(ids, token_type_ids, position_ids, inputs_embeds)
        lens = self._dev_i32(lengths)
        km = self._key_mask(key_mask, B, S)
        self._live_encode = None
        with torch.cuda.device(self.device):
            hid = torch.empty((B, S, self.cfg.hidden_size), dtype=torch.float32, device=self.device)
            pk = self._packing(packing, B, S)
            hs = at = None
            if layers is not None:
                hs, at = self._alloc_layer_outputs(B, S, layers.get("hidden_states", False), layers.get("attentions", False))
            lo, keep = self._layer_outputs(hs, at, B, S)
            self._entry(encoder_entry("encode", layers is not None, ein is not None, km is not None),
                        dict(ids=ids, inputs=ein, key_mask=km, lengths=lens, B=B, S=S, packing=pk, hidden=hid, layers=lo))
            del keep
        self._encode_serial = getattr(self, "_encode_serial", 0) + 1
        self._live_encode = (ids, lens, packing, B, S, ein, keep_in, km)   # (holds the tensors the backward reads again)
        self._last_encoder_call = (int(B), int(S), lens, packing)
        return hid if layers is None else (hid, hs, at)

    def encode_bwd(self, d_hidden, d_below=None, want_d_inputs_embeds=False, d_pooled=None):
        """Backward of the live ``encode`` from ``d_hidden`` = d(loss)/d(hidden), fp32 [B,S,H] (values at pad positions
        are ignored): the encoder range of ``self.grads`` is overwritten, the phoneme head's is zeroed and the next
        ``adamw_step`` leaves the head alone (plb_encode_bwd). ``d_below`` (plb_encode_bwd_layers): a list of L entries,
        ``d_below[l]`` = d(loss)/d(hidden_states[l]) fp32 [B,S,H] or None; ``d_hidden`` may then be None (a zero gradient
        at the last slot). ``want_d_inputs_embeds`` (plb_encode_bwd_inputs): returns fp32 [B,S,embedding_size], the gradient
        of the pre-LayerNorm embedding sum per token (zeros at pad positions) — the gradient of ``inputs_embeds``, or the
        per-phoneme saliency of a call that took ids. The key mask of an ``encode(key_mask=...)`` is taken from the live
        record (plb_encode_bwd_masked). ``d_pooled`` (plb_encode_bwd_pooled): d(loss)/d(pooler_output) fp32 [B,H] — the
        pooler backward joins the call: the pooler's range of ``self.grads`` is overwritten, position 0 of every sample
        receives its share, and the next optimizer step covers the pooler; ``d_hidden`` may then be None."""
        live = getattr(self, "_live_encode", None)
        if live is None:
            raise RuntimeError("encode_bwd: no live encode() on this engine (one backward per encode)")
        ids, lens, packing, B, S, ein, keep_in, km = live
        shape = (B, S, self.cfg.hidden_size)

        def dev(g, what):
            if g is None:
                return None
            d = torch.as_tensor(g)
            if d.dtype != torch.float32 or d.device != self.device or not d.is_contiguous():
                d = d.to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(d.shape) != shape:
                raise ValueError(f"{what} must be {list(shape)}, got {tuple(d.shape)}")
            return d

        d = dev(d_hidden, "d_hidden")
        dp = None
        if d_pooled is not None:
            dp = torch.as_tensor(d_pooled)
            if dp.dtype != torch.float32 or dp.device != self.device or not dp.is_contiguous():
                dp = dp.to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(dp.shape) != (B, self.cfg.hidden_size):
                raise ValueError(f"d_pooled must be {[B, self.cfg.hidden_size]}, got {tuple(dp.shape)}")
            if dp.data_ptr() % 16:   # (a view into a larger buffer: the engine takes 16-byte aligned gradients)
                dp = dp.clone()
        if d_below is None and d is None and dp is None:
            raise ValueError("encode_bwd: d_hidden is None and no d_below is given")
        below = None if d_below is None else [dev(g, f"d_below[{l}]") for l, g in enumerate(d_below)]
        self._live_encode = None
        with torch.cuda.device(self.device):
            pk = self._packing(packing, B, S)
            arr = None if below is None else self._ptr_array(below, self.cfg.num_hidden_layers, "d_below", shape)
            die = (torch.empty((B, S, self.cfg.embedding_size), dtype=torch.float32, device=self.device)
                   if want_d_inputs_embeds else None)
            self._entry(encoder_entry("encode_bwd", None, ein is not None, km is not None, below, want_d_inputs_embeds,
                                      dp is not None),
                        dict(ids=ids, inputs=ein, key_mask=km, lengths=lens, B=B, S=S, packing=pk, d_hidden=d, d_below=arr,
                             d_inputs_embeds=die, d_pooled=dp))
            del keep_in
        return die

    def pooler(self, hidden):
        """tanh(pooler(hidden[:, 0])) (modeling_albert.py:403), fp32 [B,H]; ``hidden`` fp32 [B,S,H] on the device."""
        self._ensure_synced()
        B, S, H = hidden.shape
        with torch.cuda.device(self.device):
            out = torch.empty((B, H), dtype=torch.float32, device=self.device)
            _lib.check(self.L.plb_pooler(self.handle, hidden.data_ptr(), B, S, out.data_ptr(), self._stream()), "plb_pooler")
        return out

    def loss_fwd(self, masked_ids, labels, lengths, idx_offsets, idx_flat, n_masked, token_ids=None, packing=None):
        """Loss of one batch WITHOUT the backward (validate(), train.py:288-304; process_batch under no_grad):
        plb_loss_fwd — the gradient buffer is not touched. Returns the 1-element device loss tensor."""
        return self._loss_call(False, masked_ids, labels, lengths, idx_offsets, idx_flat, n_masked, token_ids, packing)

    def loss_fwd_bwd(self, masked_ids, labels, lengths, idx_offsets, idx_flat, n_masked, token_ids=None, packing=None):
        """Loss of one batch + gradients of every trainable parameter into ``self.grads``.
        Returns the 1-element device tensor holding the loss (no host sync).
        With ``token_ids`` (int64 [B,S], the 4-tuple Collater's first element) the step is dual-head:
        loss = phoneme loss + token loss, ``self.loss_parts`` holds the two terms and the token head's
        gradients are produced too.
        ``packing`` (PackingPlan of these lengths, loss_fwd too): the call runs on the valid tokens only
        (include/plbert.h: plb_loss_fwd_bwd_packed). Calls in fp8 mode run padded all the same unless ``set_packed_fp8``
        is on, and so do dual-head calls unless ``set_packed_dual`` is on (plb_loss_fwd_bwd_dual_packed)."""
        return self._loss_call(True, masked_ids, labels, lengths, idx_offsets, idx_flat, n_masked, token_ids, packing)

    def _loss_call(self, backward, masked_ids, labels, lengths, idx_offsets, idx_flat, n_masked, token_ids, packing=None):
        if backward and not self.train_mode:
            raise RuntimeError("this HipEngine was built with train=False (inference / validation only)")
        self.raise_if_failed()   # a step that completed since the last call and timed out: never train on top of it
        self._ensure_synced()
        masked_ids = self._dev_i64(masked_ids)
        labels = self._dev_i64(labels)
        B, S = masked_ids.shape
        lens = self._dev_i32(lengths)
        offs = self._dev_i32(idx_offsets)
        flat = self._dev_i32(idx_flat)
        tok = None
        if token_ids is not None:
            if not self.num_tokens:
                raise ValueError("token_ids given but the engine was built without a token head (num_tokens = 0)")
            tok = self._dev_i64(token_ids)
            if tok.shape != masked_ids.shape:
                raise ValueError("token_ids must have the shape of the phoneme batch")
        with torch.cuda.device(self.device):
            pk = self._packing(packing, B, S)
            self._entry(loss_entry(backward, tok is not None, pk is not None),
                        dict(masked_ids=masked_ids, labels=labels, token_ids=tok, lengths=lens, idx_offsets=offs,
                             idx_flat=flat if n_masked else None, n_masked=int(n_masked), B=B, S=S, packing=pk, loss=self._loss,
                             loss_parts=self._loss_parts if tok is not None else None))
        self._last_loss_call = (int(B), int(n_masked), tok is not None)
        self._last_encoder_call = (int(B), int(S), lens, packing)   # (token_report: the tensors that call was given)
        return self._loss

    # ---- masked-phoneme evaluation (include/plbert.h: plb_masked_report) ---------------------------------
    # output name -> (dtype, shape as a function of (n_masked, B, topk, num_phonemes))
    REPORT_OUTPUTS = {
        "pred": (torch.int32, lambda n, B, k, V: (n,)), "rank": (torch.int32, lambda n, B, k, V: (n,)),
        "nll": (torch.float32, lambda n, B, k, V: (n,)),
        "topk_ids": (torch.int32, lambda n, B, k, V: (n, k)), "topk_logprob": (torch.float32, lambda n, B, k, V: (n, k)),
        "logits": (torch.float32, lambda n, B, k, V: (n, V)),
        "sample_loss": (torch.float32, lambda n, B, k, V: (B,)), "sample_top1": (torch.int32, lambda n, B, k, V: (B,)),
        "sample_topk": (torch.int32, lambda n, B, k, V: (B,)),
        "totals": (torch.int32, lambda n, B, k, V: (4,)), "token_totals": (torch.int32, lambda n, B, k, V: (2,)),
    }

    def masked_report(self, offsets, topk=5, want=("totals",), out=None):
        """Accuracy, top-k and losses of the LAST ``loss_fwd`` / ``loss_fwd_bwd`` call of this engine, from the logits that
        call left on the device (plb_masked_report). ``offsets``: the call's CSR offsets; ``want``: names of
        ``REPORT_OUTPUTS`` — per masked row (CSR order) pred / rank / nll / topk_ids / topk_logprob / logits, per sample
        sample_loss / sample_top1 / sample_topk, totals = [rows, top-1 correct, top-k correct, samples with rows] and, after a
        dual-head call, token_totals = [valid positions, positions whose target ties the token head's maximum]. Returns
        {name: device tensor}; only what is asked for is allocated (``out``: {name: tensor} to write into instead), nothing
        is read back. Available until the next loss call, an optimizer step in between included."""
        last = getattr(self, "_last_loss_call", None)
        if last is None:
            raise RuntimeError("masked_report: no loss call has run on this engine")
        B, n, _ = last
        unknown = [w for w in want if w not in self.REPORT_OUTPUTS]
        if unknown:
            raise ValueError(f"masked_report: unknown output(s) {unknown}; the outputs are {sorted(self.REPORT_OUTPUTS)}")
        offs = self._dev_i32(offsets)
        res, rep = {}, _lib.PlbMaskedReport()
        with torch.cuda.device(self.device):
            for name in want:
                dtype, shape = self.REPORT_OUTPUTS[name]
                shp = shape(n, B, int(topk), self.num_phonemes)
                t = out.get(name) if out else None
                if t is None:
                    t = torch.empty(shp, dtype=dtype, device=self.device)
                elif t.dtype != dtype or tuple(t.shape) != shp or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"masked_report: out[{name!r}] must be a contiguous {dtype} tensor of shape {shp} on {self.device}")
                res[name] = t
                setattr(rep, name, t.data_ptr() if t.numel() else None)
            _lib.check(self.L.plb_masked_report(self.handle, None if offs is None else offs.data_ptr(), B, int(topk),
                                                C.byref(rep), self._stream()), "plb_masked_report")
        return res

    # ---- token-head predictions without logits (include/plbert.h: plb_token_report) ----------------------------
    # output name -> (dtype, shape as a function of (n, topk, num_tokens))
    TOKEN_REPORT_OUTPUTS = {
        "topk_ids": (torch.int32, lambda n, k, V: (n, k)), "topk_logprob": (torch.float32, lambda n, k, V: (n, k)),
        "lse": (torch.float32, lambda n, k, V: (n,)), "target_logprob": (torch.float32, lambda n, k, V: (n,)),
        "target_pos": (torch.int32, lambda n, k, V: (n,)), "logits": (torch.float32, lambda n, k, V: (n, V)),
        "totals": (torch.int32, lambda n, k, V: (3,)),
    }

    def token_report(self, positions=None, token_ids=None, topk=5, want=("topk_ids", "topk_logprob"), out=None):
        """What the token head predicts on the final hidden state of the LAST call of this engine that ran the encoder —
        ``forward`` (``want_*`` all False outputs nothing else), ``encode``, ``loss_fwd`` / ``loss_fwd_bwd`` (a dual-head call,
        or a phoneme-only one that did not prune) — from one fused GEMM + top-k pass that stores no logits
        (plb_token_report). ``positions``: None = every position of [B,S] in order (a pad position has no row: ids -1,
        log-probabilities -inf, never counted), or ``(offsets, flat)``, the CSR position lists of the loss calls.
        ``token_ids`` (int64 [B,S]): the targets, needed for target_logprob / target_pos / totals. ``want``: names of
        ``TOKEN_REPORT_OUTPUTS`` — per position topk_ids / topk_logprob [n, topk], lse, target_logprob, target_pos [n],
        logits [n, num_tokens] (small n), and totals = [positions counted, target first (exact top-1), target in the top-k].
        Returns {name: device tensor}; only what is asked for is allocated (``out``: {name: tensor} to write into), nothing
        is read back. Available until the next call that runs the encoder or moves the weights (``adamw_step``,
        ``sync_weights``, ``broadcast_params``): a training loop asks between the loss call and the optimizer step."""
        last = getattr(self, "_last_encoder_call", None)
        if last is None:
            raise RuntimeError("token_report: no call has run the encoder on this engine")
        B, S, lens, packing = last
        unknown = [w for w in want if w not in self.TOKEN_REPORT_OUTPUTS]
        if unknown:
            raise ValueError(f"token_report: unknown output(s) {unknown}; the outputs are {sorted(self.TOKEN_REPORT_OUTPUTS)}")
        offs = flat = None
        n = B * S
        if positions is not None:
            offs, flat = self._dev_i32(positions[0]), self._dev_i32(positions[1])
            n = int(flat.numel())
        tok = None if token_ids is None else self._dev_i64(token_ids)
        if tok is not None and tuple(tok.shape) != (B, S):
            raise ValueError(f"token_report: token_ids must be [{B}, {S}], got {tuple(tok.shape)}")
        res, rep = {}, _lib.PlbTokenReport()
        p = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(self.device):
            for name in want:
                dtype, shape = self.TOKEN_REPORT_OUTPUTS[name]
                shp = shape(n, int(topk), self.num_tokens)
                t = out.get(name) if out else None
                if t is None:
                    t = torch.empty(shp, dtype=dtype, device=self.device)
                elif t.dtype != dtype or tuple(t.shape) != shp or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"token_report: out[{name!r}] must be a contiguous {dtype} tensor of shape {shp} on {self.device}")
                res[name] = t
                setattr(rep, name, t.data_ptr() if t.numel() else None)
            pk = self._packing(packing, B, S)
            _lib.check(self.L.plb_token_report(self.handle, p(lens), p(offs), p(flat) if n else None, n, B, S,
                                               None if pk is None else C.byref(pk), p(tok), int(topk), C.byref(rep),
                                               self._stream()), "plb_token_report")
        return res

    @property
    def loss_parts(self):
        """(phoneme loss, token loss) of the last dual-head call, on the device."""
        return self._loss_parts

    @property
    def token_range(self):
        """[start, end) of token_predictor.{weight,bias} in the flat buffers (empty without a token head)."""
        if not self.num_tokens:
            return (self.total, self.total)
        return (self.layout["token_predictor.weight"][0], self.total)

    def adamw_step(self, step, lr=7e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, grad_scale=1.0, norm_buf=None):
        """plb_adamw_step; with ``norm_buf`` (what ``grad_norm`` returned) plb_adamw_step_clipped: the gradient is
        multiplied by the clipping coefficient the device holds there, and the update is left out when the norm was not
        finite."""
        self._bind()
        with torch.cuda.device(self.device):
            if norm_buf is None:
                _lib.check(self.L.plb_adamw_step(self.handle, lr, betas[0], betas[1], eps, weight_decay, int(step),
                                                 grad_scale, self._stream()), "plb_adamw_step")
            else:
                _lib.check(self.L.plb_adamw_step_clipped(self.handle, lr, betas[0], betas[1], eps, weight_decay, int(step),
                                                         grad_scale, norm_buf.data_ptr(), self._stream()),
                           "plb_adamw_step_clipped")
        self._synced_version = self.params._version

    # ---- parameter groups and frozen tensors (include/plbert.h: plb_adamw_plan, plb_adamw_step_groups) ----
    @staticmethod
    def _groups_c(groups, group_of):
        """The C arrays of ``groups`` (dicts with lr, betas, eps, weight_decay) and ``group_of``: a sequence of
        PLB_NPARAM group indices in flat-buffer order (-1: frozen), or a dict {state-dict name: index} (absent: frozen)."""
        garr = (_lib.PlbAdamWGroup * max(1, len(groups)))()
        for k, g in enumerate(groups):
            garr[k] = _lib.PlbAdamWGroup(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                         float(g["weight_decay"]))
        return garr, HipEngine._group_of_c(group_of)

    @staticmethod
    def _group_of_c(group_of):
        if isinstance(group_of, dict):
            unknown = sorted(set(group_of) - set(_lib.PLB_PARAM_NAMES))
            if unknown:
                raise ValueError(f"group_of names no tensor of the flat layout: {unknown}")
            group_of = [group_of.get(n, -1) for n in _lib.PLB_PARAM_NAMES]
        if len(group_of) != _lib.PLB_NPARAM:
            raise ValueError(f"group_of needs {_lib.PLB_NPARAM} entries (flat-buffer order), not {len(group_of)}")
        return (C.c_int32 * _lib.PLB_NPARAM)(*[int(k) for k in group_of])

    def adamw_plan(self, step, groups, group_of):
        """plb_adamw_plan (host only; the engine need not be bound): the live segments the next ``adamw_step_groups`` with
        these arguments would launch, as a list of dicts (begin, end, group, step and the seven fp32 scalars)."""
        garr, gof = self._groups_c(groups, group_of)
        segs = (_lib.PlbAdamWSegment * _lib.PLB_NPARAM)()
        n = C.c_int32()
        _lib.check(self.L.plb_adamw_plan(self.handle, garr, len(groups), gof, int(step), segs, C.byref(n)), "plb_adamw_plan")
        return [{name: getattr(segs[i], name) for name, _ in _lib.PlbAdamWSegment._fields_} for i in range(n.value)]

    def adamw_step_groups(self, step, groups, group_of, grad_scale=1.0, norm_buf=None):
        """plb_adamw_step_groups: ``adamw_step`` with one set of hyper-parameters per group and frozen tensors, still one
        launch per range. ``groups`` / ``group_of``: see ``_groups_c``. ``norm_buf``: what ``grad_norm`` returned (the
        clipped update), or None."""
        self._bind()
        garr, gof = self._groups_c(groups, group_of)
        with torch.cuda.device(self.device):
            _lib.check(self.L.plb_adamw_step_groups(self.handle, garr, len(groups), gof, int(step), float(grad_scale),
                                                    None if norm_buf is None else norm_buf.data_ptr(), self._stream()),
                       "plb_adamw_step_groups")
        self._synced_version = self.params._version

    # ---- LAMB (include/plbert.h: plb_lamb_plan, plb_lamb_step) ----
    @staticmethod
    def _lamb_groups_c(groups, group_of):
        """``_groups_c`` for LAMB: every group dict also carries ``adapt`` (truthy: the trust ratio is on; absent: on)."""
        garr = (_lib.PlbLambGroup * max(1, len(groups)))()
        for k, g in enumerate(groups):
            garr[k] = _lib.PlbLambGroup(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                        float(g["weight_decay"]), int(bool(g.get("adapt", True))))
        return garr, HipEngine._group_of_c(group_of)

    @property
    def lamb_buf(self):
        """The engine's own LAMB buffer (plb_lamb_floats floats): [wn, un, trust, live] per tensor of the flat layout as
        the last ``lamb_step`` left them, then the partial sums."""
        if getattr(self, "_lamb_buf", None) is None:
            with torch.cuda.device(self.device):
                self._lamb_buf = torch.zeros(int(self.L.plb_lamb_floats(self.handle)), dtype=torch.float32, device=self.device)
        return self._lamb_buf

    def lamb_plan(self, step, groups, group_of):
        """plb_lamb_plan (host only; the engine need not be bound): one dict per tensor the next ``lamb_step`` with these
        arguments would step (begin, end, tensor, group, step, adapt and the eight fp32 scalars), never merged."""
        garr, gof = self._lamb_groups_c(groups, group_of)
        segs = (_lib.PlbLambSegment * _lib.PLB_NPARAM)()
        n = C.c_int32()
        _lib.check(self.L.plb_lamb_plan(self.handle, garr, len(groups), gof, int(step), segs, C.byref(n)), "plb_lamb_plan")
        return [{name: getattr(segs[i], name) for name, _ in _lib.PlbLambSegment._fields_} for i in range(n.value)]

    def lamb_step(self, step, groups, group_of, grad_scale=1.0, norm_buf=None):
        """plb_lamb_step: Adam with a per-tensor trust ratio (the definition: include/plbert.h), two streaming passes and a
        finish launch per range, nothing read back. ``groups`` / ``group_of``: see ``_groups_c``, every group with its
        ``adapt``. ``norm_buf``: what ``grad_norm`` returned (the clipped update), or None. The norms and ratios of this
        step are in ``trust_ratios()``."""
        self._bind()
        garr, gof = self._lamb_groups_c(groups, group_of)
        self._lamb_live = {s["tensor"] for s in self.lamb_plan(step, groups, group_of)}   # (host only: what this step steps)
        with torch.cuda.device(self.device):
            _lib.check(self.L.plb_lamb_step(self.handle, garr, len(groups), gof, int(step), float(grad_scale),
                                            None if norm_buf is None else norm_buf.data_ptr(), self.lamb_buf.data_ptr(),
                                            self._stream()), "plb_lamb_step")
        self._synced_version = self.params._version

    def trust_ratios(self):
        """{state-dict name: (wn, un, trust)} of the last ``lamb_step`` — 0-dim DEVICE tensors, views of ``lamb_buf``:
        nothing is read back unless the caller reads them. Tensors the step left alone (frozen, without a gradient) are
        absent; which they are is host knowledge (the plan), not a read of the buffer's ``live`` flags."""
        res = self.lamb_buf[:4 * _lib.PLB_NPARAM].view(_lib.PLB_NPARAM, 4)
        live = getattr(self, "_lamb_live", None)
        return {n: (res[i, 0], res[i, 1], res[i, 2]) for i, n in enumerate(_lib.PLB_PARAM_NAMES)
                if n in self.layout and (live is None or i in live)}

    # ---- gradient accumulation and global-norm clipping (include/plbert.h: plb_grad_accum_add, plb_grad_norm) ----
    GRAD_FIRST, GRAD_ADD, GRAD_LAST = 0, 1, 2

    @property
    def norm_buf(self):
        """The engine's own norm buffer (plb_grad_norm_floats floats, zero-filled once): [0] total norm, [1] clipping
        coefficient, [2] 1.0 when the norm was not finite, [3] updates left out for that reason; then the partial sums."""
        if getattr(self, "_norm_buf", None) is None:
            with torch.cuda.device(self.device):
                self._norm_buf = torch.zeros(int(self.L.plb_grad_norm_floats(self.handle)), dtype=torch.float32,
                                             device=self.device)
        return self._norm_buf

    def grad_accum_add(self, phase, want_partials=False):
        """Fold the gradients of the last backward call into the accumulation window: ``phase`` GRAD_FIRST / GRAD_ADD /
        GRAD_LAST (after LAST ``self.grads`` holds the window's sum). The accumulator (a second gradient-sized buffer) is
        allocated and bound by the first call. ``want_partials`` (LAST only): the pass also leaves the partial sums of
        squares in ``self.norm_buf`` for ``grad_norm(have_partials=True)``."""
        self._bind()
        with torch.cuda.device(self.device):
            if getattr(self, "_accum", None) is None:
                self._accum = torch.zeros(self.total, dtype=torch.float32, device=self.device)
                _lib.check(self.L.plb_grad_accum_bind(self.handle, self._accum.data_ptr()), "plb_grad_accum_bind")
            nb = self.norm_buf.data_ptr() if want_partials else None
            _lib.check(self.L.plb_grad_accum_add(self.handle, int(phase), nb, self._stream()), "plb_grad_accum_add")

    def grad_norm(self, grad_scale=1.0, max_norm=0.0, have_partials=False, group_of=None):
        """Global norm of the gradients the next ``adamw_step`` covers, times ``grad_scale``, and the coefficient of
        torch.nn.utils.clip_grad_norm_ for ``max_norm`` (<= 0: no clipping), on the device (plb_grad_norm). Returns
        ``self.norm_buf``; its first four floats are the result. Nothing is read back. ``group_of`` (see
        ``adamw_step_groups``): the norm of the tensors that are not frozen only (plb_grad_norm_groups; one pass over the
        gradients, ``have_partials`` does not combine with it)."""
        self._bind()
        with torch.cuda.device(self.device):
            nb = self.norm_buf
            if group_of is not None:
                if have_partials:
                    raise ValueError("grad_norm: the partial sums of a LAST add cover frozen tensors too: have_partials "
                                     "does not combine with group_of")
                _lib.check(self.L.plb_grad_norm_groups(self.handle, self._group_of_c(group_of), float(grad_scale),
                                                       float(max_norm or 0.0), nb.data_ptr(), self._stream()),
                           "plb_grad_norm_groups")
                return nb
            _lib.check(self.L.plb_grad_norm(self.handle, float(grad_scale), float(max_norm or 0.0), nb.data_ptr(),
                                            int(bool(have_partials)), self._stream()), "plb_grad_norm")
        return nb
