"""Training-step driver of the hot path: the loop body of the reference (train.py:350-357) as three
device calls — loss+backward (plb_loss_fwd_bwd), gradient all-reduce (RCCL via torch.distributed,
only when world_size > 1), AdamW (plb_adamw_step).

Data parallelism follows the reference's DDP semantics: one process per GPU,
replicated parameters and optimizer state, each rank normalises its loss by its LOCAL count of
non-empty samples (train.py:129) and gradients are averaged over ranks; the logged loss is the
local one (train.py:395-410).
"""
from __future__ import annotations

from dataclasses import dataclass

import os

import numpy as np
import torch

from .data import masked_indices_to_csr
from .dist import GradReducer
from .engine import HipEngine, PackingPlan
from .init import reference_init_state_dict


@dataclass
class StagedBatch:
    """One collated batch resident on the device (what dataloader.py:297 returns, staged once)."""
    masked: torch.Tensor          # int64 [B,S]
    labels: torch.Tensor          # int64 [B,S]
    lengths: torch.Tensor | None  # int32 [B] or None when nothing is padded
    offsets: torch.Tensor         # int32 [B+1]
    flat: torch.Tensor            # int32 [n_masked]
    n_masked: int
    n_tokens: int
    token_ids: torch.Tensor | None = None  # int64 [B,S]: grapheme-token targets of the 4-tuple Collater (dual-head)
    packing: PackingPlan | None = None     # token-packed execution: the plan of these lengths (engine.PackingPlan), or None
    lengths_host: np.ndarray | None = None  # the collater's lengths as it returned them (host): a plan can be made later


def packed_default():
    """PLBERT_PACKED=1: ragged batches run token-packed (include/plbert.h: PlbPacking) wherever ``packed`` is left open."""
    return os.environ.get("PLBERT_PACKED", "0") == "1"


def make_packing(lengths, S, device, packed=None):
    """The PackingPlan of a batch when packing is on (``packed``; None = PLBERT_PACKED) and saves rows, else None. Host
    arithmetic plus one small asynchronous upload of the row table: nothing is read back from the device."""
    if not (packed_default() if packed is None else packed) or lengths is None:
        return None
    plan = PackingPlan(lengths, S)
    return plan.to(device) if plan.packed else None


def validate_token_ids(token_ids, shape, lengths, num_tokens):
    """Targets of the token head must be class ids at every valid position (the kernel indexes with them)."""
    tok = np.asarray(token_ids)
    if tok.shape != tuple(shape):
        raise ValueError("token_ids must have the shape of the phoneme batch")
    valid = np.arange(shape[1])[None, :] < np.asarray(lengths)[:, None]
    if tok[valid].min(initial=0) < 0 or tok[valid].max(initial=0) >= num_tokens:
        raise ValueError("token id outside [0, num_tokens)")


def validate_batch(labels, masked, lengths, masked_indices, vocab_size):
    """Host checks the kernels rely on (they index without bounds checks)."""
    labels = np.asarray(labels)
    masked = np.asarray(masked)
    if labels.shape != masked.shape or labels.ndim != 2:
        raise ValueError("labels / masked must both be [B,S]")
    B, S = masked.shape
    if len(lengths) != B or len(masked_indices) != B:
        raise ValueError("lengths / masked_indices must have one entry per sample")
    if masked.min(initial=0) < 0 or masked.max(initial=0) >= vocab_size or labels.min(initial=0) < 0 or \
            labels.max(initial=0) >= vocab_size:
        raise ValueError("phoneme id outside the vocabulary")
    for b, (L, idx) in enumerate(zip(lengths, masked_indices)):
        if not (1 <= int(L) <= S):
            raise ValueError(f"sample {b}: length {L} outside [1, {S}]")
        if len(idx):
            a = np.asarray(idx)
            if a.min() < 0 or a.max() >= int(L):
                raise ValueError(f"sample {b}: masked index outside [0, length)")
            if len(np.unique(a)) != len(a):
                raise ValueError(f"sample {b}: duplicate masked index")


def _rewind_steps(owner):
    """HandoffTimeout callback for an object that counts optimizer steps (``step_count``): the device skipped
    ``err.skipped_updates`` of them. Holds the owner weakly (the engine must not keep its trainer alive)."""
    import weakref
    ref = weakref.ref(owner)

    def cb(err):
        o = ref()
        if o is not None:
            o.step_count = max(0, o.step_count - err.skipped_updates)
            first = getattr(o, "_first_step", None)
            if first:   # tensors whose first update was one of the skipped ones were never updated
                for n in [n for n, at in first.items() if at > o.step_count]:
                    del first[n]
                o._noted.clear()
    return cb


def _note_stepped(owner, engine, groups, group_of, liveness=None):
    """Before a grouped update at ``owner.step_count``: remember the tensors it updates for the first time
    (``owner._first_step``: {state-dict name: step count of its first update}; a tensor that is not in it has no optimizer
    state). Which of ``group_of``'s tensors the engine steps is the plan's answer (plb_adamw_plan); it is asked once per
    membership and ``liveness`` (what the caller knows of the engine's has-a-gradient state), not once per step."""
    key = (frozenset(group_of), liveness)
    if key in owner._noted:
        return
    for n in planned_names(engine, engine.adamw_plan(owner.step_count, groups, group_of)):
        owner._first_step.setdefault(n, owner.step_count)
    owner._noted.add(key)


def _clip_norm(owner, engine, grad_scale, **which):
    """With ``owner.max_grad_norm``: the norm and clipping coefficient of the gradients the next update consumes, on the
    device (``engine.grad_norm``; ``which``: have_partials or group_of). Returns the norm buffer for the update and keeps
    its four result floats as ``owner.last_grad_norm``; None when clipping is off."""
    if owner.max_grad_norm is None:
        return None
    norm_buf = engine.grad_norm(grad_scale, owner.max_grad_norm, **which)
    owner.last_grad_norm = norm_buf[:4]
    return norm_buf


_POOLER_NAMES = ("encoder.pooler.weight", "encoder.pooler.bias")

# torch.optim.AdamW's group keys beside the hyper-parameters, at its defaults: what its state_dict carries in every group
TORCH_ADAMW_EXTRA = {"amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                     "fused": None, "decoupled_weight_decay": True}


def _scatter_state(engine, selection):
    """``selection`` ({state-dict name: torch's {step, exp_avg, exp_avg_sq}}) into the flat moment buffers, zeroed first; the
    pooler (which has state once a ``train_pooler`` encoder has stepped it) shares the count of the encoder. Returns (names written, step count outside the token head, the token head's; 0:
    none). The fused update keeps ONE count each: differing counts are refused before anything is written."""
    e = engine
    ta = e.token_range[0]
    kept, steps, tok_steps = [], set(), set()
    for n, st in selection.items():
        off, size, _ = e.layout[n]
        is_tok = bool(e.num_tokens) and off >= ta
        kept.append(n)
        (tok_steps if is_tok else steps).add(int(float(st["step"])))
    if len(steps) > 1 or len(tok_steps) > 1:
        raise ValueError(f"per-parameter step counts differ ({sorted(steps)} / token head {sorted(tok_steps)}): "
                         "the fused AdamW keeps one step for the encoder + phoneme head and one for the token head")
    e.exp_avg.zero_()
    e.exp_avg_sq.zero_()
    for n in kept:
        off, size, shp = e.layout[n]
        e.exp_avg[off:off + size].view(shp).copy_(selection[n]["exp_avg"])
        e.exp_avg_sq[off:off + size].view(shp).copy_(selection[n]["exp_avg_sq"])
    return kept, (steps.pop() if steps else 0), (tok_steps.pop() if tok_steps else 0)


class PLBertTrainer:
    """PhonemeOnlyModel + AdamW(lr) of train.py:266-272 on one GPU, optionally data parallel.
    ``num_tokens > 0`` builds MultiTaskModel's second head (model.py:11); batches staged with ``token_ids``
    then train both heads (loss = phoneme loss + token loss, see include/plbert.h plb_loss_fwd_bwd_dual)."""

    def __init__(self, cfg, num_phonemes, max_batch=32, max_seq=512, lr=7e-5, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.01, device=None, seed=0, state_dict=None, process_group=None, force_collectives=False,
                 num_tokens=0, comm="auto", overlap=True, packed=None, packed_dual=None, packed_fp8=None,
                 max_grad_norm=None, track_accuracy=False, no_decay=(), frozen=(), optimizer="adamw",
                 exclude_from_layer_adaptation=("bias", "LayerNorm", "layer_norm")):
        """``optimizer``: "adamw" (the default: nothing changes) or "lamb" — Adam with a per-tensor trust ratio, the
        optimizer of large-batch BERT / ALBERT pre-training (include/plbert.h: plb_lamb_step holds the definition; the
        weight decay is then INSIDE the update). Every optimizer step is plb_lamb_step: two streaming passes and a finish
        launch per range, norms and ratios stay on the device (``engine.trust_ratios()``). Tensors whose name holds a
        substring of ``exclude_from_layer_adaptation`` step with trust ratio 1. Composes with ``no_decay``, ``frozen``,
        ``max_grad_norm``, ``step_accumulated``, packed and fp8 modes, which all sit before or behind the optimizer step.
        Data-parallel runs need no further collective: the norms are taken over all-reduced gradients and replicated
        parameters and are identical on every rank.
        ``no_decay`` / ``frozen`` (tuples of substrings matched against state-dict names; both empty, the default: the
        single plb_adamw_step of before): tensors whose name holds a ``no_decay`` substring are updated with weight decay 0
        — the usual BERT recipe is ``("bias", "LayerNorm", "layer_norm")`` here: the layer's second LayerNorm is named
        ``full_layer_layer_norm``, which ``"LayerNorm"`` alone does not match —, tensors whose name holds a ``frozen`` substring are not updated
        at all and keep their moments, and a clipped step takes its norm over the tensors that are not frozen
        (plb_adamw_step_groups / plb_grad_norm_groups: still one launch per range). ``param_groups`` then holds the groups'
        live dicts (``weight_decay``, ``names``, and any of lr / betas / eps that should differ from the trainer's own).
        ``track_accuracy`` (default off: a step then launches what it launched before): every ``step`` also launches the
        totals-only report on its loss call's masked rows (plb_masked_report) and keeps ``last_accuracy`` — a device int32 [4]:
        masked rows, top-1 correct, top-5 correct, samples that have rows; ``step_accumulated``: summed over its micro-steps —
        the way ``last_grad_norm`` is kept: nothing is read back.
        ``max_grad_norm`` (None or <= 0: off): every optimizer step clips the global norm of its mean gradient to this value
        as torch.nn.utils.clip_grad_norm_ does, on the device (plb_grad_norm + plb_adamw_step_clipped); ``last_grad_norm``
        then holds [norm, coefficient, not-finite flag, updates left out] as a device tensor. Nothing is read back.
        ``packed``: ragged batches run on their valid tokens only (token-packed execution, include/plbert.h PlbPacking);
        None = PLBERT_PACKED=1. Steps in fp8 mode run padded all the same unless ``packed_fp8`` is on (None =
        PLBERT_PACKED_FP8=1; include/plbert.h plb_set_packed_fp8), and so do dual-head steps unless ``packed_dual`` is on
        (None = PLBERT_PACKED_DUAL=1; plb_set_packed_dual): both only have an effect together with ``packed``.
        ``comm``: how the gradient exchange of a data-parallel run travels.
        "rccl"  — the engine's own RCCL communicator behind the C ABI (plb_comm_init / plb_allreduce_grads): the
                  all-reduce is issued by plb_loss_fwd_bwd itself, piece by piece on the engine's communication
                  stream while the remaining weight-gradient GEMMs run (``overlap``); torch.distributed only
                  carries the 128-byte unique id. Needs one GPU per rank.
        "torch" — ``torch.distributed.all_reduce`` on the flat buffer (dist.GradReducer): gloo in the CPU / shared-GPU
                  tests, or any backend the caller initialised.
        "auto"  — "rccl" when the process group spans more than one rank (or ``force_collectives``) and every rank of
                  this node has a GPU of its own, else "torch"."""
        self.engine = HipEngine(cfg, num_phonemes, num_tokens, max_batch=max_batch, max_seq=max_seq, device=device)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.step_count = 0
        self.no_decay, self.frozen = tuple(no_decay), tuple(frozen)
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, not {optimizer!r}")
        self.optimizer = optimizer
        self.exclude_from_layer_adaptation = tuple(exclude_from_layer_adaptation)
        self.param_groups = None     # parameter groups (no_decay / frozen): a list of live dicts; None: one plb_adamw_step
        self._first_step = {}        # ... and the tensors a grouped step has updated: {name: step count of the first update}
        self._noted, self._dual = set(), False   # (_note_stepped's memo; whether the step in hand is a dual-head one)
        if self.no_decay or self.frozen:
            self.param_groups = name_param_groups(self.engine.layout, weight_decay, self.no_decay, self.frozen)
        if optimizer == "lamb":   # always grouped: the groups' dicts carry ``adapt`` beside ``weight_decay`` and ``names``
            self.param_groups = lamb_param_groups(self.engine.layout, weight_decay, self.no_decay, self.frozen,
                                                  self.exclude_from_layer_adaptation)
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm is not None and float(max_grad_norm) > 0 else None
        self.last_grad_norm = None   # the four result floats of the last clipped step (device)
        self.track_accuracy = bool(track_accuracy)
        self.last_accuracy = None    # int32 [4] of the last step's masked rows (device; track_accuracy)
        self.packed = packed_default() if packed is None else bool(packed)
        if packed_dual is not None:   # (None: the engine has read PLBERT_PACKED_DUAL itself)
            self.engine.set_packed_dual(packed_dual)
        self.packed_dual = self.engine.packed_dual
        if packed_fp8 is not None:    # (None: the engine has read PLBERT_PACKED_FP8 itself)
            self.engine.set_packed_fp8(packed_fp8)
        self.packed_fp8 = self.engine.packed_fp8
        self.reducer = GradReducer(process_group, device=self.engine.device, force=force_collectives)
        self.world = self.reducer.world
        sd = state_dict if state_dict is not None else reference_init_state_dict(cfg, num_phonemes, num_tokens, seed=seed)
        self.engine.load_state_dict(sd)
        # a step whose fused LayerNorm hand-off timed out is skipped on the device (include/plbert.h: plb_status) and
        # raises HandoffTimeout from the next engine call: the bias-correction count goes back by the skipped updates
        self.engine._on_handoff_timeout.append(_rewind_steps(self))
        self.comm = "none"
        self._overlap = False
        if self.reducer.active:
            if comm == "auto":   # PLBERT_COMM=rccl|torch overrides (tests: the engine's own exchange through a stand-in library)
                comm = os.environ.get("PLBERT_COMM") or ("rccl" if own_gpu_per_rank() else "torch")
            if comm == "rccl":
                uid = exchange_unique_id(HipEngine.comm_unique_id if self.reducer.rank == 0 else None, process_group)
                self.engine.comm_init(uid, self.reducer.rank, self.world)
                self.engine.set_grad_overlap(overlap)
                self._overlap = bool(overlap)
                self.engine.broadcast_params(0)  # DDP's start-up broadcast of rank 0's parameters
            elif comm == "torch":
                self.reducer.broadcast_(self.engine.params)
                self.engine.sync_weights()
            else:
                raise ValueError(f"comm must be 'auto', 'rccl' or 'torch', not {comm!r}")
            self.comm = comm

    def packing_of(self, batch):
        """The batch's packing plan: the one it was staged with, else (packing on) one made now from its host lengths."""
        if batch.packing is None and self.packed and batch.lengths is not None and batch.lengths_host is not None:
            batch.packing = make_packing(batch.lengths_host, batch.masked.shape[1], self.engine.device, True)
        return batch.packing if self.packed else None

    def stage_batch(self, labels, masked, lengths, masked_indices, validate=True, token_ids=None, packed=None):
        """``stage_reference_batch`` on this trainer's engine; ``packed`` None: the trainer's own setting."""
        batch = (labels, masked, lengths, masked_indices)
        return stage_reference_batch(self.engine, batch if token_ids is None else (token_ids, *batch), validate,
                                     self.packed if packed is None else packed)

    def loss_and_grads(self, batch: StagedBatch):
        return self.engine.loss_fwd_bwd(batch.masked, batch.labels, batch.lengths, batch.offsets, batch.flat,
                                        batch.n_masked, token_ids=batch.token_ids, packing=self.packing_of(batch))

    def loss_only(self, batch: StagedBatch):
        """validate() (train.py:288-304): the batch's loss without the backward."""
        return self.engine.loss_fwd(batch.masked, batch.labels, batch.lengths, batch.offsets, batch.flat, batch.n_masked,
                                    token_ids=batch.token_ids, packing=self.packing_of(batch))

    ACCURACY_TOPK = 5

    def evaluate(self, batch: StagedBatch, topk=5):
        """``loss_only`` plus the report on its masked rows (plb_masked_report): {'loss': the batch's loss (1 element),
        'totals': int32 [4] = masked rows, top-1 correct, top-``topk`` correct, samples that have rows, 'sample_loss' /
        'sample_top1' / 'sample_topk': [B], and after a dual-head batch 'token_totals': int32 [2] = valid positions, positions
        whose target ties the token head's maximum, and 'token_exact': int32 [3] = valid positions, positions whose target is
        the token head's first class (the lowest index wins a tie), positions whose target is among its first ``topk``
        (plb_token_report)}, all on the device."""
        loss = self.loss_only(batch).clone()
        want = ("totals", "sample_loss", "sample_top1", "sample_topk") + (("token_totals",) if batch.token_ids is not None else ())
        res = {"loss": loss, **self.engine.masked_report(batch.offsets, topk=topk, want=want)}
        if batch.token_ids is not None:
            res["token_exact"] = self.engine.token_report(None, batch.token_ids, topk=topk, want=("totals",))["totals"]
        return res

    def _track(self, batch, first=True):
        """The totals of the loss call that has just run, into ``last_accuracy`` (``first``) or added to it."""
        if self.last_accuracy is None:
            self.last_accuracy = torch.zeros(4, dtype=torch.int32, device=self.engine.device)
        if first:
            self.engine.masked_report(batch.offsets, topk=self.ACCURACY_TOPK, out={"totals": self.last_accuracy})
        else:
            self.last_accuracy.add_(self.engine.masked_report(batch.offsets, topk=self.ACCURACY_TOPK)["totals"])

    def all_reduce_grads(self, dual=False):
        """Sum the trainable gradient range over ranks (RCCL over xGMI, one collective in the step's stream:
        see dist.GradReducer); the AdamW kernel applies the 1/world factor. A dual-head step also carries
        the token head's gradients."""
        if self.comm == "rccl":
            self.engine.allreduce_grads()  # joins the pieces plb_loss_fwd_bwd issued (or reduces now: overlap off)
            return
        self.reducer.all_reduce_(self.engine.grads[: self.engine.trainable])
        if dual:
            a, b = self.engine.token_range
            self.reducer.all_reduce_(self.engine.grads[a:b])
        if self.reducer.active:  # the health word travels with the gradients: every rank skips a poisoned update, or none
            self.engine.status_exchange(self.reducer.all_reduce_)

    def step(self, batch: StagedBatch):
        """zero_grad + backward + optimizer.step of train.py:355-357; returns the local loss (device).
        HandoffTimeout (never observed; engine.py) is raised by the engine call that follows the failed step's completion
        on the device: the failed step's update has been left out on EVERY rank (the health word is agreed between the
        ranks inside the step) and all replicas are bit-identical, so the caller may run the batch again. A loop that
        reads each loss back (run.train_loop) sees it exactly at the failed step, on every rank at the same step; a
        loop that does not may see it one step late and — in a data-parallel run — at different steps on different
        ranks: such a caller must treat it as the end of the run (resume from the replicas, which are consistent)."""
        loss = self.loss_and_grads(batch)
        if self.track_accuracy:
            self._track(batch)
        dual = batch.token_ids is not None
        if batch.n_masked == 0 and self.world == 1 and not dual:
            return loss  # reference: zero-loss fallback has no graph, the optimizer sees no gradients
        self.all_reduce_grads(dual)
        self._dual = dual
        self._optimizer_step(1.0 / self.world)
        return loss

    def optimizer_entry_points(self):
        """The C entry points (include/plbert.h) an optimizer step of this trainer calls, in order: host knowledge of
        ``_optimizer_step``'s dispatch, no device."""
        grouped = self.param_groups is not None
        norm = () if self.max_grad_norm is None else ("plb_grad_norm_groups" if grouped else "plb_grad_norm",)
        if self.optimizer == "lamb":
            return norm + ("plb_lamb_step",)
        if grouped:
            return norm + ("plb_adamw_step_groups",)
        return norm + ("plb_adamw_step_clipped" if norm else "plb_adamw_step",)

    def _optimizer_step(self, grad_scale, have_partials=False):
        """AdamW (or LAMB: ``optimizer``) on what the gradient buffer holds; with ``max_grad_norm`` the norm (taken after
        the exchange, so every rank computes the same coefficient) and the clipped update."""
        self.step_count += 1
        if self.param_groups is not None:
            groups, group_of = self.groups_for_step()
            # (a LAST add's partial sums cover frozen tensors too: the grouped norm is one pass of its own)
            norm_buf = _clip_norm(self, self.engine, grad_scale, group_of=group_of)
            _note_stepped(self, self.engine, groups, group_of, liveness=self._dual)
            step = self.engine.lamb_step if self.optimizer == "lamb" else self.engine.adamw_step_groups
            step(self.step_count, groups, group_of, grad_scale=grad_scale, norm_buf=norm_buf)
            return
        norm_buf = _clip_norm(self, self.engine, grad_scale, have_partials=have_partials)
        self.engine.adamw_step(self.step_count, self.lr, self.betas, self.eps, self.weight_decay, grad_scale=grad_scale,
                               norm_buf=norm_buf)

    @property
    def stepped(self):
        """The tensors a grouped step has updated (or a checkpoint brought state for): the others have no optimizer state.
        An update the device left out (HandoffTimeout) does not count."""
        return set(self._first_step)

    def mark_stepped(self, names, reset=False):
        """Count ``names`` as updated before the first step (a checkpoint's tensors with state)."""
        if reset:
            self._first_step = {}
        self._noted.clear()
        for n in names:
            self._first_step[n] = 0

    def groups_for_step(self):
        """(groups, group_of) of a grouped step: every group's hyper-parameters (the trainer's own where its dict names
        none) and {state-dict name: group index} (a name in no group is frozen)."""
        base = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        groups = [{**base, **{k: v for k, v in g.items() if k != "names"}} for g in self.param_groups]
        return groups, {n: k for k, g in enumerate(self.param_groups) for n in g["names"]}

    def step_accumulated(self, batches):
        """ONE optimizer step over a list of staged batches (gradient accumulation, include/plbert.h plb_grad_accum_add):
        every batch is one loss + backward call, their gradients are summed on the device and the update uses their mean,
        ``grad_scale = 1 / (world * len(batches))``. A data-parallel run exchanges ONCE, after the last micro-step (the
        engine's own communicator runs with overlap off for the duration). Returns the mean of the micro-step losses as
        a 1-element device tensor. A window in which no micro-step has a masked position (single rank, phoneme-only)
        does not step, like ``step``."""
        batches = list(batches)
        if not batches:
            raise ValueError("step_accumulated needs at least one batch")
        if len(batches) == 1:
            return self.step(batches[0])
        eng = self.engine
        k = len(batches)
        rccl_overlap = self.comm == "rccl" and self._overlap
        if rccl_overlap:
            eng.set_grad_overlap(False)
        try:
            dual = False
            loss_sum = None
            clip_local = self.max_grad_norm is not None and not self.reducer.active and self.param_groups is None
            for i, b in enumerate(batches):
                loss = self.loss_and_grads(b)
                if self.track_accuracy:
                    self._track(b, first=i == 0)
                loss_sum = loss.clone() if loss_sum is None else loss_sum.add_(loss)
                dual = dual or b.token_ids is not None
                last = i == k - 1
                eng.grad_accum_add(eng.GRAD_FIRST if i == 0 else eng.GRAD_LAST if last else eng.GRAD_ADD,
                                   want_partials=last and clip_local)
            loss_sum.mul_(1.0 / k)
            if all(b.n_masked == 0 for b in batches) and self.world == 1 and not dual:
                return loss_sum
            self.all_reduce_grads(dual)
            self._dual = dual
            self._optimizer_step(1.0 / (self.world * k), have_partials=clip_local)
        finally:
            if rccl_overlap:
                eng.set_grad_overlap(True)
        return loss_sum


def name_param_groups(layout, weight_decay, no_decay=(), frozen=()):
    """The groups of PLBertTrainer(no_decay=..., frozen=...) over the state-dict names of ``layout``: [{'weight_decay':
    weight_decay, 'names': [...]}, {'weight_decay': 0.0, 'names': [...]}] (a group without names is left out); a name that
    holds a ``frozen`` substring is in no group. ValueError when ``frozen`` leaves nothing to train. Pure: no device, no
    engine."""
    decay, plain = [], []
    for n in layout:
        if any(f in n for f in frozen):
            continue
        (plain if any(d in n for d in no_decay) else decay).append(n)
    groups = [g for g in ({"weight_decay": weight_decay, "names": decay}, {"weight_decay": 0.0, "names": plain}) if g["names"]]
    if not groups:
        raise ValueError(f"frozen={tuple(frozen)!r} matches every parameter name: nothing would be trained")
    return groups


OPTIMIZERS = ("adamw", "lamb")


def lamb_param_groups(layout, weight_decay, no_decay=(), frozen=(), exclude=()):
    """``name_param_groups`` for PLBertTrainer(optimizer="lamb"): every group is cut in two by the layer adaptation — a name
    that holds an ``exclude`` substring steps with trust ratio 1 (``adapt`` False) — so a group's dict is {'weight_decay',
    'names', 'adapt'}. Pure: no device, no engine."""
    out = []
    for g in name_param_groups(layout, weight_decay, no_decay, frozen):
        off = [n for n in g["names"] if any(x in n for x in exclude)]
        on = [n for n in g["names"] if n not in off]
        out += [{"weight_decay": g["weight_decay"], "names": names, "adapt": adapt} for names, adapt in ((on, True), (off, False))
                if names]
    return out


def planned_names(engine, plan):
    """The state-dict names of the tensors inside the segments of an ``engine.adamw_plan``."""
    return {n for n, (off, size, _) in engine.layout.items() if any(s["begin"] <= off and off + size <= s["end"] for s in plan)}


def resolve_param_groups(layout, named_parameters, groups):
    """torch's ``param_groups`` (dicts whose 'params' are Parameters of ONE model) -> (group_of, frozen): group_of = {layout
    name: group index} of every tensor a group holds, frozen = the layout names of the model's parameters that are in no
    group or have ``requires_grad == False`` (they are not updated and keep their moments). ``layout``: the engine's
    {state-dict name: ...}; ``named_parameters``: the model's (a stand-alone AlbertModel names its parameters without the
    "encoder." prefix of the layout). Q, K and V are separate tensors of the layout and may sit in different groups. Pure:
    no device. Raises ValueError for a parameter in two groups (torch's wording) and for one that is not the model's."""
    by_id = {}
    for n, p in named_parameters:
        by_id[id(p)] = (n if n in layout else "encoder." + n, p)
    group_of = {}
    for k, g in enumerate(groups):
        params = g["params"]
        params = [params] if isinstance(params, torch.Tensor) else list(params)
        for p in params:
            if id(p) not in by_id:
                raise ValueError(f"param group {k} holds a parameter that is not one of the model's: the fused optimizer "
                                 "updates the model's flat parameter buffer and nothing else")
            name = by_id[id(p)][0]
            if name not in layout:
                raise ValueError(f"param group {k}: {name!r} is no tensor of the engine's flat layout")
            if name in group_of:
                raise ValueError("some parameters appear in more than one parameter group")
            group_of[name] = k
    frozen = [n for n, p in by_id.values() if n in layout and (n not in group_of or not p.requires_grad)]
    for n in frozen:
        group_of.pop(n, None)
    return group_of, frozen


def own_gpu_per_rank():
    """True when every rank launched on this node can have a GPU to itself (RCCL refuses two ranks on one device)."""
    import os
    import torch.distributed as dist
    local_world = os.environ.get("LOCAL_WORLD_SIZE")
    if local_world is None:  # not under a launcher: assume every rank of the group lives on this node
        local_world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    return torch.cuda.device_count() >= int(local_world)


_uid_round = [0]


def exchange_unique_id(make, group=None):
    """Rank 0 of ``group`` creates the RCCL unique id (``make()``), everyone receives its 128 bytes. Over the
    process group's key-value store when there is one (no device traffic, so torch creates no communicator of its
    own), else as a broadcast object."""
    import torch.distributed as dist
    rank = dist.get_rank(group)
    store = None
    if group is None:
        try:
            store = dist.distributed_c10d._get_default_store()
        except Exception:
            store = None
    if store is not None:
        key = f"plbert_rccl_uid_{_uid_round[0]}"
        _uid_round[0] += 1
        if rank == 0:
            store.set(key, make())
        return bytes(store.get(key))
    box = [make() if rank == 0 else None]
    dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    return bytes(box[0])


# ---- drop-in forms of the reference's step functions ---------------------------------------------------
class _FusedLoss(torch.autograd.Function):
    """Bridges the fused fwd+bwd call into autograd so the reference loop body
    ``loss = process_batch(...); optimizer.zero_grad(); accelerator.backward(loss); optimizer.step()``
    (train.py:352-357) runs unchanged: forward computes loss AND gradients in one engine call,
    backward hands each Parameter its slice of the engine's flat gradient buffer."""

    @staticmethod
    def forward(ctx, engine, names, batch, *params):
        loss = engine.loss_fwd_bwd(batch.masked, batch.labels, batch.lengths, batch.offsets, batch.flat, batch.n_masked,
                                   token_ids=batch.token_ids, packing=batch.packing)
        ctx.engine, ctx.names, ctx.dual = engine, names, batch.token_ids is not None
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        eng = ctx.engine
        ta, tb = eng.token_range
        grads = []
        for n in ctx.names:
            off, size, shp = eng.layout[n]
            has = off + size <= eng.trainable or (ctx.dual and off >= ta)  # pooler: never; token head: dual steps
            grads.append(eng.grads[off:off + size].view(shp) if has else None)
        # d(loss)/d(param) is already in the flat buffer; scale by the upstream gradient on the device
        # (1.0 for loss.backward(); no host sync to find out)
        eng.grads[: eng.trainable].mul_(grad_out)
        if ctx.dual:
            eng.grads[ta:tb].mul_(grad_out)
        return (None, None, None, *grads)


def stage_reference_batch(engine, batch, validate=True, packed=None):
    """(labels, masked, lengths, masked_indices) as PhonemeOnlyCollater returns it, or the 5-tuple
    (token_ids, labels, masked, lengths, masked_indices) of Collater (dataloader.py:200-223) -> StagedBatch.
    ``packed`` (None = PLBERT_PACKED): the same padded tensors plus the packing plan of a ragged batch."""
    token_ids = None
    if len(batch) == 5:
        token_ids, *batch = batch
    labels, masked, lengths, idx = batch
    if validate:
        validate_batch(labels, masked, lengths, idx, engine.cfg.vocab_size)
        if token_ids is not None:
            validate_token_ids(token_ids, np.asarray(masked).shape, lengths, engine.num_tokens)
    dev = engine.device
    masked_t = torch.as_tensor(np.asarray(masked), dtype=torch.int64).to(dev)
    labels_t = torch.as_tensor(np.asarray(labels), dtype=torch.int64).to(dev)
    S = masked_t.shape[1]
    lens = np.asarray(lengths, dtype=np.int32)
    lengths_t = None if (lens == S).all() else torch.from_numpy(lens).to(dev)
    off, flat = masked_indices_to_csr(idx)
    tok_t = None if token_ids is None else torch.as_tensor(np.asarray(token_ids), dtype=torch.int64).to(dev)
    plan = None if lengths_t is None else make_packing(lens, S, dev, packed)
    return StagedBatch(masked_t, labels_t, lengths_t, torch.from_numpy(off).to(dev), torch.from_numpy(flat).to(dev),
                       int(off[-1]), int(lens.sum()), tok_t, plan, lens)


def device_mask_batch(labels, lengths=None, seed=1, step=0, word_pred_prob=0.15, phoneme_mask_prob=0.8, replace_prob=0.1,
                      device=None):
    """Fast mode of the masking path: word-level mask / replace / keep ON THE DEVICE
    (plb_mask_batch). Same decision tree and probabilities as MaskedPhonemeDataset (dataloader.py:83-108),
    Philox randomness keyed by (seed, step, sample, word): distribution-matched, not the reference's bit
    stream. ``labels`` int64 [B,S] = unmasked phoneme ids with the separator 186 after each word, zero
    padded; returns a StagedBatch (one small device->host read for the masked count)."""
    import ctypes as C

    from . import _lib
    from .symbols import MASK_ID, SEPARATOR_ID

    L = _lib.lib()
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    labels_t = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).to(dev, torch.int64).contiguous()
    B, S = labels_t.shape
    lengths_t = None
    if lengths is not None:
        lens = np.asarray(lengths, dtype=np.int32)
        lengths_t = None if (lens == S).all() else torch.from_numpy(lens).to(dev)
    masked = torch.empty_like(labels_t)
    offsets = torch.empty(B + 1, dtype=torch.int32, device=dev)
    flat = torch.empty(B * S, dtype=torch.int32, device=dev)
    scratch = torch.empty(B + B * S, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(L.plb_mask_batch(labels_t.data_ptr(), None if lengths_t is None else lengths_t.data_ptr(), B, S,
                                int(seed), int(step), word_pred_prob, phoneme_mask_prob, replace_prob, MASK_ID,
                                SEPARATOR_ID, masked.data_ptr(), offsets.data_ptr(), flat.data_ptr(), scratch.data_ptr(),
                                stream), "plb_mask_batch")
    n = int(offsets[B].item())
    n_tokens = int(B * S if lengths is None else np.asarray(lengths).sum())
    return StagedBatch(masked, labels_t, lengths_t, offsets, flat[:n], n, n_tokens)


def device_apply_mask(records, device=None, word_separator=None):
    """Bit-exact masking through the GPU: ``records`` are ``MaskedPhonemeDataset.decisions(i)``
    dicts — the reference's random draws, made on the host in the reference's order — and plb_apply_mask does the
    integer work (crop, mask / replace, separator handling, index re-basing, zero padding, length-descending batch
    order) on the device. Returns (StagedBatch, labels, masked, lengths, token_ids|None): identical to what
    ``PhonemeOnlyCollater()([ds[i] ...])`` / ``Collater()`` return (tests/test_gpu_apply_mask.py)."""
    import ctypes as C

    from . import _lib
    from .data import collate_decisions
    from .symbols import MASK_ID

    L = _lib.lib()
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    c = collate_decisions(records)
    B, S = c["B"], c["S"]
    if B < 1 or S < 1:
        raise ValueError("device_apply_mask needs at least one non-empty sample")
    with torch.cuda.device(dev):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
        ids, repl = up(c["ids"]), up(c["repl"])
        sample_off, word_off = up(c["sample_off"]), up(c["word_off"])
        word_begin, word_len, action = up(c["word_begin"]), up(c["word_len"]), up(c["action"])
        crop = up(c["crop_start"])
        wtok = None if c["word_token"] is None else up(c["word_token"])
        labels = torch.empty((B, S), dtype=torch.int64, device=dev)
        masked = torch.empty_like(labels)
        tokens = torch.empty_like(labels) if wtok is not None else None
        lens = torch.empty(B, dtype=torch.int32, device=dev)
        offsets = torch.empty(B + 1, dtype=torch.int32, device=dev)
        flat = torch.empty(B * S, dtype=torch.int32, device=dev)
        scratch = torch.empty(B + B * S, dtype=torch.int32, device=dev)
        p = lambda t: None if t is None else t.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(L.plb_apply_mask(ids.data_ptr(), sample_off.data_ptr(), word_off.data_ptr(), word_begin.data_ptr(),
                                    word_len.data_ptr(), action.data_ptr(), repl.data_ptr(), p(wtok),
                                    int(word_separator if word_separator is not None else 0), crop.data_ptr(), B, S,
                                    MASK_ID, labels.data_ptr(), masked.data_ptr(), p(tokens), lens.data_ptr(),
                                    offsets.data_ptr(), flat.data_ptr(), scratch.data_ptr(), stream), "plb_apply_mask")
        n = int(offsets[B].item())
    lengths = c["lengths"]
    lengths_t = None if all(l == S for l in lengths) else lens
    return StagedBatch(masked, labels, lengths_t, offsets, flat[:n], n, int(sum(lengths)), tokens), labels, masked, lengths, tokens


def process_batch(model, batch, criterion=None, accelerator=None):
    """train.py:381-390 — ``batch = (phoneme_labels, masked_phonemes, input_lengths, masked_indices)``.
    ``criterion`` / ``accelerator`` are accepted for signature compatibility: the loss is the
    reference's calculate_phoneme_loss with nn.CrossEntropyLoss() (train.py:107-131, 215), computed by
    the HIP engine. Returns a 0-dim tensor; under autograd its ``backward()`` fills ``param.grad``.
    A 5-tuple batch (Collater, dataloader.py:200-223: token_ids first) on a MultiTaskModel trains both heads:
    phoneme loss + token loss (plb_loss_fwd_bwd_dual)."""
    engine = model.engine
    staged = batch if isinstance(batch, StagedBatch) else stage_reference_batch(engine, batch)
    if staged.n_masked == 0 and staged.token_ids is None:  # train.py:129
        return torch.tensor(0.0, device=engine.device, requires_grad=True)
    names, params = [], []
    for n, p in model.named_parameters():
        names.append(n)
        params.append(p)
    if torch.is_grad_enabled():
        return _FusedLoss.apply(engine, names, staged, *params)
    # validate() (train.py:288-304): forward + loss only; the gradient buffer is left alone
    return engine.loss_fwd(staged.masked, staged.labels, staged.lengths, staged.offsets, staged.flat,
                           staged.n_masked, token_ids=staged.token_ids, packing=staged.packing)[0].clone()


class AdamW:
    """``torch.optim.AdamW(model.parameters(), lr=...)`` of train.py:272 as one fused HIP launch over the
    model's flat buffers. ``params`` must be the parameters of ONE plbert_amd model (it identifies the
    engine); state_dict()/load_state_dict() carry step + both moments (train.py:417-421 'optimizer').
    ``params`` may also be torch's iterable of dicts ({"params": [...], "lr": ..., "betas": ..., "eps": ...,
    "weight_decay": ...}; missing keys inherit the defaults): every group steps with its own hyper-parameters, a model
    parameter in no group — or with ``requires_grad == False``, or whose ``.grad`` is None at ``step()`` — is frozen (not
    updated, moments untouched), and the update is still one launch per range (plb_adamw_step_groups). One step count is
    shared by all tensors outside the token head: a tensor thawed later continues with it (include/plbert.h)."""

    HYPER = ("lr", "betas", "eps", "weight_decay")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, model=None, max_grad_norm=None):
        """``max_grad_norm`` (None or <= 0: off): ``step`` clips the global norm of the gradients it consumes (times
        ``grad_scale``) as torch.nn.utils.clip_grad_norm_ does, on the device; ``last_grad_norm`` holds [norm, coefficient,
        not-finite flag, updates left out] as a device tensor."""
        params = list(params)
        self._groups = None          # dict groups: torch's live list of dicts; None: one group, today's path
        if params and isinstance(params[0], dict):
            self._groups = []
            pending, params = params, [p for _, p in model.named_parameters()] if model is not None else []
        self.param_list = params
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm is not None and float(max_grad_norm) > 0 else None
        self.last_grad_norm = None
        if model is None:
            raise ValueError("pass model=<PhonemeOnlyModel|MultiTaskModel|AlbertModel(finetune=True)>: the fused optimizer updates the model's "
                             "flat parameter buffer")
        self.engine = model.engine
        self.defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.step_count = 0
        self._pool_stepped = False   # the ungrouped step has covered the pooler (state_dict then holds its moments)
        self.grad_scale = 1.0
        self.engine._on_handoff_timeout.append(_rewind_steps(self))
        # (a stand-alone AlbertModel names its parameters without the "encoder." prefix of the engine's layout)
        by_id = {id(p): (n if n in self.engine.layout else "encoder." + n) for n, p in model.named_parameters()}
        self._names = [by_id[id(p)] for p in self.param_list]
        if self._groups is not None:
            self._model = model
            self._first_step = {}    # {name: step count of its first update}: the others have no entry in state_dict()['state']
            self._resolved = (None, None)   # resolve_param_groups' result for the membership it was made from
            self._noted = set()             # _note_stepped's memo
            for g in pending:
                self.add_param_group(g)

    @property
    def param_groups(self):
        """One group, and its dict IS the live ``defaults``: ``for g in optimizer.param_groups: g['lr'] = ...`` (the
        reference README's fine-tuning set-up) takes effect at the next step. Built from dicts: the live list of the
        groups' dicts, as in torch."""
        return [self.defaults] if self._groups is None else self._groups

    def add_param_group(self, group):
        """torch.optim.Optimizer.add_param_group: a further dict of parameters that are in no group yet (it thaws them)."""
        if self._groups is None:
            raise ValueError("add_param_group needs an optimizer built from parameter-group dicts")
        if not isinstance(group, dict) or "params" not in group:
            raise ValueError("a parameter group is a dict with a 'params' entry")
        g = dict(group)
        g["params"] = [g["params"]] if isinstance(g["params"], torch.Tensor) else list(g["params"])
        for k in self.HYPER:
            g.setdefault(k, self.defaults[k])
        resolve_param_groups(self.engine.layout, self._model.named_parameters(), self._groups + [g])   # raises
        self._groups.append(g)

    def _live_groups(self):
        """(groups, group_of) of this step: requires_grad and .grad are read now."""
        key = (tuple(tuple(map(id, g["params"])) for g in self._groups), tuple(p.requires_grad for p in self.param_list))
        if self._resolved[0] != key:   # (membership changes with the groups and with requires_grad only)
            self._resolved = (key, resolve_param_groups(self.engine.layout, self._model.named_parameters(), self._groups)[0])
        group_of = self._resolved[1]
        grads = {n: p.grad for n, p in zip(self._names, self.param_list)}
        return self._groups, {n: k for n, k in group_of.items() if grads.get(n) is not None}

    def _step_groups(self):
        e = self.engine
        groups, group_of = self._live_groups()
        if not group_of:
            return
        for n, p in zip(self._names, self.param_list):   # (as in step(): whatever .grad holds now is what the update consumes)
            off, size, shp = e.layout[n]
            if n in group_of and p.grad.data_ptr() != e.grads.data_ptr() + 4 * off:
                e.grads[off:off + size].view(shp).copy_(p.grad)
        self.step_count += 1
        norm_buf = _clip_norm(self, e, self.grad_scale, group_of=group_of)
        _note_stepped(self, e, groups, group_of)
        self._fused_step(groups, group_of, norm_buf)

    def _fused_step(self, groups, group_of, norm_buf):
        self.engine.adamw_step_groups(self.step_count, groups, group_of, self.grad_scale, norm_buf=norm_buf)

    def zero_grad(self, set_to_none=True):
        for p in self.param_list:
            p.grad = None

    def step(self):
        # parameters without a gradient are skipped as torch does: a step with no gradient at all (the
        # zero-loss fallback) changes nothing; otherwise the trainable range is updated in one launch
        if all(p.grad is None for p in self.param_list):
            return
        if self._groups is not None:
            return self._step_groups()
        e = self.engine
        for n, p in zip(self._names, self.param_list):
            # autograd may have handed the Parameter a copy of its gradient slice (or user code replaced
            # / clipped .grad): whatever .grad holds now is what the fused update must consume
            off, size, shp = e.layout[n]
            if p.grad is not None and p.grad.data_ptr() != e.grads.data_ptr() + 4 * off:
                e.grads[off:off + size].view(shp).copy_(p.grad)
            if p.grad is not None and n in _POOLER_NAMES:
                self._pool_stepped = True   # (a train_pooler backward: the engine steps the pooler with this count)
        self.step_count += 1
        d = self.defaults
        e.adamw_step(self.step_count, d["lr"], d["betas"], d["eps"], d["weight_decay"], self.grad_scale,
                     norm_buf=_clip_norm(self, e, self.grad_scale))

    def state_dict(self):
        """torch.optim.AdamW layout ({'state': {index: {step, exp_avg, exp_avg_sq}}, 'param_groups': [...]}) with
        parameter indices in ``model.parameters()`` order, so the 'optimizer' entry of a checkpoint
        (train.py:417-421) can be loaded by either implementation. Parameters that never received a
        gradient (the pooler without ``train_pooler``; the token head before its first dual-head step) have no state, as in
        torch; the token head carries its own step count (it may have started later than the encoder), the pooler shares
        the encoder's."""
        e = self.engine
        d = self.defaults
        state = {}
        ta = e.token_range[0]
        tok_steps = e.token_head_steps
        for i, n in enumerate(self._names):
            off, size, shp = e.layout[n]
            if off + size <= e.trainable:
                steps = self.step_count
            elif off >= ta and e.num_tokens:
                steps = tok_steps
            else:   # the pooler: state once a step has covered it
                steps = self.step_count if self._groups is not None or self._pool_stepped else 0
            if self._groups is not None and n not in self._first_step:
                steps = 0   # (frozen so far: torch has no state for a parameter it never stepped)
            if steps > 0:
                state[i] = {"step": torch.tensor(float(steps)),
                            "exp_avg": e.exp_avg[off:off + size].view(shp).clone(),
                            "exp_avg_sq": e.exp_avg_sq[off:off + size].view(shp).clone()}
        if self._groups is not None:   # torch's multi-group layout; indices count model.parameters() order
            index = {id(p): i for i, p in enumerate(self.param_list)}
            groups = [{**TORCH_ADAMW_EXTRA, **{k: (tuple(v) if k == "betas" else v) for k, v in g.items() if k != "params"},
                       "params": [index[id(p)] for p in g["params"]]} for g in self._groups]
            return {"state": state, "param_groups": groups}
        group = {"lr": d["lr"], "betas": tuple(d["betas"]), "eps": d["eps"], "weight_decay": d["weight_decay"],
                 **TORCH_ADAMW_EXTRA, "params": list(range(len(self.param_list)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        e = self.engine
        e._bind()
        if self._groups is not None:
            return self._load_groups(sd)
        if "param_groups" in sd:
            g = sd["param_groups"][0]
            for k in ("lr", "betas", "eps", "weight_decay"):
                if k in g:
                    self.defaults[k] = tuple(g[k]) if k == "betas" else g[k]
            kept, self.step_count, e.token_head_steps = _scatter_state(e, {self._names[int(i)]: st for i, st in sd["state"].items()})
            self._pool_stepped = any(n in _POOLER_NAMES for n in kept)
            return
        self.step_count = int(sd["step"])  # compact form written by early versions of this class
        e.exp_avg[: e.trainable].copy_(sd["exp_avg"])
        e.exp_avg_sq[: e.trainable].copy_(sd["exp_avg_sq"])

    def _load_groups(self, sd):
        """A state dict of this class or of torch.optim.AdamW with the same group sizes: every group's settings, and the
        state of saved parameter k of the groups' chain goes to this optimizer's k-th (torch's positional rule).
        ONE step count: torch counts steps per parameter, the fused update keeps one count for everything outside the token
        head (include/plbert.h). A torch state dict in which a tensor sat out a step — frozen for a while, or without a
        gradient — holds differing counts and is refused (ValueError): loading it would change the bias correction of some
        tensor. Dicts this class wrote, and torch dicts whose stepped tensors share one count, load."""
        e = self.engine
        saved = sd["param_groups"]
        if [len(g["params"]) for g in saved] != [len(g["params"]) for g in self._groups]:
            raise ValueError("loaded state dict has parameter groups of other sizes: "
                             f"{[len(g['params']) for g in saved]} against {[len(g['params']) for g in self._groups]}")
        name_of = {id(p): n for n, p in zip(self._names, self.param_list)}
        target = {}
        for gs, g in zip(saved, self._groups):
            for i, p in zip(gs["params"], g["params"]):
                target[int(i)] = name_of[id(p)]
        # (differing step counts are refused here, before anything is written: the groups' settings included)
        kept, self.step_count, e.token_head_steps = _scatter_state(e, {target[int(i)]: st for i, st in sd["state"].items()})
        for gs, g in zip(saved, self._groups):
            for k, v in gs.items():
                if k != "params":
                    g[k] = tuple(v) if k == "betas" else v
        self._first_step = {n: 0 for n in kept}
        self._noted.clear()


class Lamb(AdamW):
    """LAMB — Adam with a per-tensor trust ratio, the optimizer ALBERT was trained with — over the model's flat buffers:
    two streaming HIP passes and a finish launch per range (plb_lamb_step; include/plbert.h holds the definition, torch
    ships none). The surface of ``AdamW`` above: ``params`` (Parameters of ONE plbert_amd model, or torch's iterable of
    dicts), live ``param_groups`` / ``add_param_group``, ``zero_grad``, ``step``, ``max_grad_norm``, and ``state_dict`` /
    ``load_state_dict`` in torch's layout (``state[i] = {step, exp_avg, exp_avg_sq}``) with ``adapt`` as a group key. The
    moments are AdamW's bit for bit, so either class loads the other's state.
    ``adapt`` of a group: True / False turn the trust ratio on / off for its tensors; None (the default) decides per tensor:
    a name that holds a substring of ``exclude_from_layer_adaptation`` steps with trust ratio 1. The weight decay is inside
    the update (u = r / bc1 + weight_decay * p), so it is scaled by the trust ratio like the rest.
    ``model.engine.trust_ratios()`` has the norms and ratios of the last step as device tensors."""

    HYPER = ("lr", "betas", "eps", "weight_decay", "adapt")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, model=None, max_grad_norm=None,
                 exclude_from_layer_adaptation=("bias", "LayerNorm", "layer_norm")):
        params = list(params)
        if not (params and isinstance(params[0], dict)):
            params = [{"params": params}]   # (always grouped: a parameter that was not passed is not stepped, as in torch)
        self.exclude = tuple(exclude_from_layer_adaptation)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, model=model,
                         max_grad_norm=max_grad_norm)

    def add_param_group(self, group):
        self.defaults.setdefault("adapt", None)
        super().add_param_group(group)

    def _live_groups(self):
        """AdamW's (groups, group_of) with every group cut in two where its tensors differ in layer adaptation."""
        groups, group_of = super()._live_groups()
        cut, index, cut_of = [], {}, {}
        for n, k in group_of.items():
            adapt = groups[k].get("adapt")
            adapt = not any(x in n for x in self.exclude) if adapt is None else bool(adapt)
            if (k, adapt) not in index:
                index[k, adapt] = len(cut)
                cut.append({**groups[k], "adapt": adapt})
            cut_of[n] = index[k, adapt]
        return cut, cut_of

    def _fused_step(self, groups, group_of, norm_buf):
        self.engine.lamb_step(self.step_count, groups, group_of, self.grad_scale, norm_buf=norm_buf)

    def state_dict(self):
        sd = super().state_dict()
        sd["param_groups"] = [{k: v for k, v in g.items() if k not in TORCH_ADAMW_EXTRA} for g in sd["param_groups"]]
        return sd
