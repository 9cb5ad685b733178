"""Run management of the hot path's caller: what ``train.train(args)`` does around the step in the
reference — run directory + resume-by-directory (train.py:174-210), latest-checkpoint discovery (train.py:46-79),
validation before the first step and at every ``save_interval`` (train.py:288-336,344,369-373), ``step_N.pth`` files
(train.py:412-425) — around the MI355X-native step (``PLBertTrainer``: plb_loss_fwd_bwd -> RCCL exchange -> plb_adamw_step)
and input pipeline (``DeviceFeeder``).

Differences from the reference, on purpose: metrics go to ``<run dir>/metrics.jsonl`` and stdout instead of wandb
(out of scope); the dataset may be handed in as any sequence of ``{'phonemes': [...]}`` rows
(the reference's hub download, train.py:245, needs a network); ``num_workers`` and device-side masking are options of
``training_params`` (``num_workers``, ``device_masking``) that default to the reference's behaviour (0 / off).

    python -m plbert_amd.run --config_path configs/config.yml --run_name default        # train.py:27-32
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
from collections import deque

import numpy as np
import torch
import torch.distributed as dist
import yaml

from .checkpoint import (find_latest_checkpoint, optimizer_state_from_flat, optimizer_state_to_flat,
                         reference_param_names)
from .config import albert_config_from_yaml
from .data import build_dataloader
from .dist import init_from_env, shard_batch, world_info
from .symbols import symbols

MAX_EPOCHS = 10  # train.py:145


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config_path", type=str, default="configs/config.yml")
    ap.add_argument("--run_name", type=str, default="default")
    return vars(ap.parse_args(argv))


def setup_config_and_directories(args, config_path):
    """Run folder decides: an existing folder that holds a copy of the config RESUMES with that copy; an existing folder
    without one is cleaned of ``step_*`` files and starts fresh; otherwise the folder is created (train.py:174-210).
    Returns (config, log_dir, resuming). With several ranks only rank 0 touches the folder (the reference guards the
    same block with ``accelerator.is_main_process``, train.py:181); the others read its decision after a barrier."""
    rank, world = world_info()
    if world > 1:
        decided = [None]
        if rank == 0:
            decided[0] = _setup_run_dir(args, config_path)
        dist.broadcast_object_list(decided, src=0)
        return decided[0]
    return _setup_run_dir(args, config_path)


def _setup_run_dir(args, config_path):
    with open(config_path) as f:
        given = yaml.safe_load(f)
    log_dir = os.path.join(given["training_params"]["output_dir"], args["run_name"])
    kept = os.path.join(log_dir, os.path.basename(config_path))
    if os.path.isdir(log_dir) and os.path.exists(kept):
        with open(kept) as f:
            return yaml.safe_load(f), log_dir, True
    if os.path.isdir(log_dir):
        for name in os.listdir(log_dir):
            if name.startswith("step_"):
                os.remove(os.path.join(log_dir, name))
    os.makedirs(log_dir, exist_ok=True)
    shutil.copy(config_path, kept)
    return given, log_dir, False


class _Log:
    """Rank-0 metrics sink: one JSON object per event, to stdout and ``metrics.jsonl`` (the reference logs the same
    keys to wandb: phoneme_loss, phoneme_loss_avg, val_phoneme_loss, epoch, step — train.py:326-331,398-410)."""

    def __init__(self, log_dir, main):
        self.main = main
        self.f = open(os.path.join(log_dir, "metrics.jsonl"), "a") if main else None

    def __call__(self, **kv):
        if self.main:
            line = json.dumps(kv)
            print(line, flush=True)
            self.f.write(line + "\n")
            self.f.flush()


def _state_for_file(trainer, step, epoch):
    """``{'net','step','epoch','optimizer'}`` with the optimizer entry in torch.optim.AdamW's layout, as train.py:416-421
    writes it: state indices count the reference's ``model.parameters()`` order (checkpoint.REFERENCE_PARAM_ORDER), so
    the reference's ``optimizer.load_state_dict`` binds every moment to the tensor it belongs to."""
    eng = trainer.engine
    tok0 = eng.token_range[0]

    def steps_of(name, off, size):
        if off + size <= eng.trainable:
            return trainer.step_count
        return eng.token_head_steps if eng.num_tokens and off >= tok0 else 0

    grouped = getattr(trainer, "param_groups", None)
    if grouped is not None:   # a tensor no grouped step has updated (frozen so far) has no state, as in torch
        steps_all = steps_of
        steps_of = lambda name, off, size: steps_all(name, off, size) if name in trainer.stepped else 0
    state, n = optimizer_state_from_flat(eng.layout, eng.exp_avg, eng.exp_avg_sq, steps_of)
    extra = {"amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
             "fused": None, "decoupled_weight_decay": True}
    if grouped is None:
        groups = [{"lr": trainer.lr, "betas": tuple(trainer.betas), "eps": trainer.eps, "weight_decay": trainer.weight_decay,
                   **extra, "params": list(range(n))}]
    else:   # torch's multi-group layout: every group's settings and the indices of its tensors; a frozen tensor is in none
        index = {name: i for i, name in enumerate(reference_param_names(eng.layout))}
        groups = [{"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": g["weight_decay"], **extra,
                   **({"adapt": bool(tg["adapt"])} if "adapt" in tg else {}),   # (LAMB: the group's layer adaptation)
                   "params": [index[name] for name in tg["names"]]}
                  for g, tg in zip(trainer.groups_for_step()[0], grouped)]
    out = {"net": {k: v.cpu() for k, v in eng.state_dict().items()}, "step": step, "epoch": epoch,
           "optimizer": {"state": state, "param_groups": groups}}
    if getattr(trainer, "optimizer", "adamw") != "adamw":   # (absent = AdamW: the reference's files and every earlier one)
        out["optimizer_kind"] = trainer.optimizer
    return out


def save_checkpoint(trainer, current_step, log_dir, current_epoch, main=True):
    path = os.path.join(log_dir, f"step_{current_step}.pth")
    if main:
        torch.save(_state_for_file(trainer, current_step, current_epoch), path)
        print(f"Checkpoint saved at: {path}", flush=True)
    return path


def load_checkpoint(trainer, path, restore_groups=True):
    """Weights (``module.`` prefixes stripped, non-strict: train.py:98-100) and, when present, the AdamW state — of a
    file this driver wrote or of a reference ``step_N.pth`` (indices in ``model.parameters()`` order).
    Parameter groups (PLBertTrainer(no_decay=..., frozen=...)): what the trainer was built with always stays — learning
    rate, betas and eps come from the configuration, as they do without groups. With ``restore_groups`` (a resume) a file that
    holds several groups gives a trainer built WITHOUT groups its membership and weight decays, and a trainer built WITH
    groups must agree with it (ValueError otherwise: the run would silently continue under another recipe). A file with the
    ordinary single group (an ungrouped run, a reference checkpoint) never changes the trainer's groups.
    ``restore_groups=False`` (``pretrained_model``): the file's groups are not looked at.
    The optimizer kind (``optimizer_kind`` in the file; absent: AdamW): a resume under the other kind is refused (ValueError)
    before anything is loaded — the moments would fit, the run would silently continue under another update rule; as a
    pretrained model the file loads under either."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    eng = trainer.engine
    kind, mine_kind = ck.get("optimizer_kind", "adamw"), getattr(trainer, "optimizer", "adamw")
    if restore_groups and kind != mine_kind:
        raise ValueError(f"{path} was written under optimizer {kind!r} and this run is configured with {mine_kind!r} "
                         "(training_params.optimizer): resume with the optimizer it was written under, or load it as "
                         "model_params.pretrained_model")
    opt = ck.get("optimizer")
    saved = (opt.get("param_groups") or []) if opt else []
    file_groups = None
    if restore_groups and len(saved) > 1:
        names = reference_param_names(eng.layout)
        file_groups = [{"weight_decay": g["weight_decay"], "names": [names[int(i)] for i in g["params"]],
                        **({"adapt": g["adapt"]} if "adapt" in g else {})} for g in saved]
        mine = getattr(trainer, "param_groups", None)
        if mine is not None:
            key = lambda gs: sorted((float(g["weight_decay"]), bool(g.get("adapt", True)), tuple(sorted(g["names"]))) for g in gs)
            if key(mine) != key(file_groups):
                raise ValueError(f"{path} was written under other parameter groups than this run is configured with "
                                 "(training_params.weight_decay / no_decay / frozen): resume with the recipe it was written "
                                 "under, or load it as model_params.pretrained_model")
            file_groups = None   # (the same recipe: the trainer's own dicts stay, with whatever else they carry)
    eng.load_state_dict({k.replace("module.", ""): v for k, v in ck["net"].items()}, strict=False)
    if opt and opt.get("state"):
        tok0 = eng.token_range[0]

        def is_tok(off):
            return bool(eng.num_tokens) and off >= tok0

        steps = optimizer_state_to_flat(opt["state"], eng.layout, eng.exp_avg, eng.exp_avg_sq,
                                        lambda n, off, size: off + size <= eng.trainable or is_tok(off))  # not the pooler
        main_steps = {v for n, v in steps.items() if not is_tok(eng.layout[n][0])}
        tok_steps = {v for n, v in steps.items() if is_tok(eng.layout[n][0])}
        trainer.step_count = max(main_steps) if main_steps else 0
        eng.token_head_steps = max(tok_steps) if tok_steps else 0
        if file_groups is not None:
            trainer.param_groups = file_groups
        if getattr(trainer, "param_groups", None) is not None:
            trainer.mark_stepped(steps, reset=True)   # the tensors that have state in the file, and only they
    print(f"Checkpoint {path} loaded.", flush=True)
    return int(ck.get("step", 0))


def initialize_model(config, log_dir, resuming, device=None, max_batch=None):
    """train.py:261-286: model + AdamW(lr), optional ``pretrained_model``, then the run's latest checkpoint when
    resuming. Returns (trainer, current_step)."""
    from .train import PLBertTrainer
    cfg = albert_config_from_yaml(config, len(symbols))
    tp = config["training_params"]
    _, world = world_info()
    per_rank = max(1, int(tp["batch_size"]) // world)           # split_batches=True: batch_size is global (train.py:220)
    trainer = PLBertTrainer(cfg, num_phonemes=len(symbols), max_batch=max_batch or per_rank,
                            max_seq=int(config["dataset_params"]["max_seq_length"]), lr=float(tp["learning_rate"]),
                            device=device, packed_dual=tp.get("packed_dual"),      # (None: PLBERT_PACKED_DUAL)
                            packed_fp8=tp.get("packed_fp8"),                       # (None: PLBERT_PACKED_FP8)
                            max_grad_norm=tp.get("max_grad_norm"),                 # (not in the reference's config.yml; absent: off)
                            track_accuracy=bool(tp.get("eval_accuracy", False)),   # (likewise)
                            # (likewise) weight_decay: absent = AdamW's 0.01 on every tensor; no_decay / frozen: lists of
                            # name substrings, absent = one group and nothing frozen (PLBertTrainer)
                            weight_decay=float(tp.get("weight_decay", 0.01)), no_decay=tuple(tp.get("no_decay") or ()),
                            frozen=tuple(tp.get("frozen") or ()),
                            # (likewise) optimizer: absent = "adamw"; "lamb": plb_lamb_step, with the names excluded from
                            # the layer adaptation (absent: biases and LayerNorm)
                            optimizer=str(tp.get("optimizer", "adamw")).lower(),
                            **({"exclude_from_layer_adaptation": tuple(tp["exclude_from_layer_adaptation"])}
                               if tp.get("exclude_from_layer_adaptation") is not None else {}))
    if config["model_params"].get("pretrained_model"):
        print(f"Loading pretrained model from: {config['model_params']['pretrained_model']}")
        load_checkpoint(trainer, config["model_params"]["pretrained_model"], restore_groups=False)
    found, last = find_latest_checkpoint(log_dir)
    current_step = 0
    if found and resuming:
        current_step = load_checkpoint(trainer, os.path.join(log_dir, f"step_{last}.pth")) or last
    return trainer, current_step


def _feeder(loader, trainer, word_separator, budget=None):
    """ONE DeviceFeeder per (trainer, loader): its pinned buffers, device slots and copy stream are created once (a fresh
    set per validation pass was measured as tens of slow steps after every pass)."""
    import weakref

    from .pipeline import DeviceFeeder
    # keyed by the loader OBJECT (weakly): id() can be handed to a new loader once the old one has been collected
    cache = trainer.__dict__.setdefault("_feeders", weakref.WeakKeyDictionary())
    f = cache.get(loader)
    if f is None:
        f = cache[loader] = DeviceFeeder(loader, device=trainer.engine.device, vocab_size=trainer.engine.cfg.vocab_size,
                                         word_separator=word_separator, draw_budget=budget,
                                         packed=getattr(trainer, "packed", None))
    return f


class _ShardedLoader:
    """This rank's contiguous slice of every collated batch of ``loader`` (accelerate's split_batches=True, train.py:220 —
    ``dist.shard_batch``; a short last validation batch is completed as accelerate's even_batches=True does). An iterable
    like the loader itself, so the same DeviceFeeder (pinned buffer, copy stream, double-buffered device slots) feeds a
    data-parallel rank: every rank still draws the masks of the WHOLE global batch from its own copy of the reference's
    streams, as the reference's ranks do."""

    def __init__(self, loader, rank, world):
        self.loader, self.rank, self.world = loader, rank, world
        self.batch_size = getattr(loader, "batch_size", None)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        first = None
        for batch in self.loader:
            cur = (np.asarray(batch[0]), np.asarray(batch[1]), batch[2], batch[3])
            if first is None:
                first = cur
            yield shard_batch(cur, self.rank, self.world, pad=True, batch_size=self.batch_size, first_batch=first)


def _source(loader, trainer):
    """What this rank's feeder iterates: the loader itself on one GPU, its sharded view under a launcher (one view per
    loader, kept with the trainer so that the feeder cache — keyed by the object it iterates — finds it again)."""
    import weakref
    rank, world = world_info()
    if world == 1 or getattr(loader, "plb_per_rank", False):   # (build_dataloader(shard=...): already this rank's samples)
        return loader
    views = trainer.__dict__.setdefault("_sharded_views", weakref.WeakKeyDictionary())
    v = views.get(loader)
    if v is None:
        v = views[loader] = _ShardedLoader(loader, rank, world)
    return v


def _batches(loader, trainer, device_masking, word_separator, budget=None):
    """Collated batches of the loader as device-resident StagedBatch objects: this rank's contiguous slice of every
    global batch (accelerate's split_batches=True), copies overlapped with compute (DeviceFeeder) — on one GPU and, since
    round 5, on every rank of a data-parallel run (it staged each batch with blocking copies before).
    ``budget``: see DeviceFeeder.draw_budget (the training loader: draws are granted up to the next validation)."""
    yield from _feeder(_source(loader, trainer), trainer, word_separator, budget)


MAX_HANDOFF_RETRIES = 3


def _checked(trainer, call, note=None):
    """``float(call().item())`` with the engine's hand-off status checked right behind the read-back, where it is exact. A
    step the engine declared invalid (HandoffTimeout: NaN loss, update left out on every rank, engine reset — never
    observed) is run again, up to MAX_HANDOFF_RETRIES times; in a data-parallel run every rank sees the failure at
    the same step (the health word is agreed inside the step), so all ranks retry the same batch together."""
    from .engine import HandoffTimeout
    for attempt in range(MAX_HANDOFF_RETRIES + 1):
        try:
            loss = float(call().item())
            trainer.engine.raise_if_failed()
            return loss
        except HandoffTimeout as ex:
            if attempt == MAX_HANDOFF_RETRIES:
                raise
            if note is not None:
                note(handoff_timeout=str(ex), retry=attempt + 1)


def validate(trainer, val_loader, device_masking=False, word_separator=None):
    """Mean of the per-batch losses, forward only (train.py:288-304; masks are re-drawn each pass, as there)."""
    total, n = 0.0, 0
    for b in _batches(val_loader, trainer, device_masking, word_separator):
        total += _checked(trainer, lambda: trainer.loss_only(b))
        n += 1
    return total / max(n, 1)


def validate_metrics(trainer, val_loader, device_masking=False, word_separator=None, topk=5):
    """``validate`` plus the accuracy at the masked positions: {'val_phoneme_loss': the mean of the per-batch losses, exactly
    what ``validate`` returns, 'val_phoneme_acc', 'val_phoneme_top<topk>': MICRO-averages over the pass — correct rows
    summed over the batches, over masked rows summed over the batches (0.0 for a pass without masked rows)}. The counts of
    every batch (plb_masked_report, totals only) are added up on the device and read back once, behind the last batch.
    When the batches carry token ids (dual-head) the token head is counted too, over every valid position
    (plb_token_report, totals only, summed and read back with the others): 'val_token_acc' (the target is the head's first
    class) and 'val_token_top<topk>'. A phoneme-only pass returns the three phoneme keys alone."""
    total, n, counts, tcounts = 0.0, 0, None, None
    for b in _batches(val_loader, trainer, device_masking, word_separator):
        total += _checked(trainer, lambda: trainer.loss_only(b))
        t = trainer.engine.masked_report(b.offsets, topk=topk, want=("totals",))["totals"]
        counts = t.to(torch.int64) if counts is None else counts.add_(t)
        tok = getattr(b, "token_ids", None)
        if tok is not None:
            t = trainer.engine.token_report(None, tok, topk=topk, want=("totals",))["totals"]
            tcounts = t.to(torch.int64) if tcounts is None else tcounts.add_(t)
        n += 1
    if tcounts is not None:   # one read-back for both heads
        both = torch.cat([counts[:3], tcounts]).tolist()
        (rows, top1, topk_n), (trows, ttop1, ttopk) = (int(v) for v in both[:3]), (int(v) for v in both[3:])
    else:
        rows, top1, topk_n = (int(v) for v in counts[:3].tolist()) if counts is not None else (0, 0, 0)
    res = {"val_phoneme_loss": total / max(n, 1), "val_phoneme_acc": top1 / rows if rows else 0.0,
           f"val_phoneme_top{topk}": topk_n / rows if rows else 0.0}
    if tcounts is not None:
        res["val_token_acc"] = ttop1 / trows if trows else 0.0
        res[f"val_token_top{topk}"] = ttopk / trows if trows else 0.0
    return res


class _AccReader:
    """The masked-row counts of a step (``trainer.last_accuracy``, overwritten by the next step), read back the way
    ``_LossReader`` reads the loss: copied into one of two pinned host buffers on the step's stream, waited for by event."""

    def __init__(self, trainer):
        import torch
        self.torch, self.trainer = torch, trainer
        self.host = [torch.zeros(4, dtype=torch.int32).pin_memory() for _ in range(2)]
        self.events = [torch.cuda.Event() for _ in range(2)]
        self.n = 0

    @staticmethod
    def ratio(counts):
        rows, top1 = int(counts[0]), int(counts[1])
        return top1 / rows if rows else 0.0

    def post(self):
        k = self.n & 1
        self.n += 1
        self.host[k].copy_(self.trainer.last_accuracy, non_blocking=True)
        self.events[k].record(self.torch.cuda.current_stream(self.trainer.engine.device))
        return k

    def read(self, k):
        self.events[k].synchronize()
        return self.ratio(self.host[k])

    def now(self):
        """Behind a loss that has just been read back with ``.item()``: the stream is idle, the counts are this step's."""
        return self.ratio(self.trainer.last_accuracy.tolist())


class _LossReader:
    """Read a step's loss back WITHOUT stalling the step behind it: ``post`` copies the engine's one-element loss buffer
    (overwritten by the next step) into one of two pinned host words on the step's stream and records an event;
    ``read`` waits for that event only — by then the next step is already enqueued, so the GPU never waits for the host
    to come back from a read-back (measured with the real pipeline, 4 workers, profiles/r05_train_loop_loss_readback_*.jsonl:
    9.57 -> 9.24 ms per step in bf16, 8.04 -> 7.77 in fp8 — the fed step without any read-back: 9.25 / 7.79)."""

    def __init__(self, device):
        import torch
        self.torch, self.device = torch, device
        self.host = [torch.zeros(1).pin_memory() for _ in range(2)]
        self.events = [torch.cuda.Event() for _ in range(2)]
        self.n = 0

    def post(self, loss_dev):
        k = self.n & 1
        self.n += 1
        self.host[k].copy_(loss_dev, non_blocking=True)
        self.events[k].record(self.torch.cuda.current_stream(self.device))
        return k

    def read(self, k):
        self.events[k].synchronize()
        return float(self.host[k][0])


class _NormReader:
    """The gradient norm of a clipped step (``trainer.last_grad_norm[0]``, overwritten by the next step), read back the way
    ``_LossReader`` reads the loss: copied into one of two pinned host words on the step's stream, waited for by event."""

    def __init__(self, trainer):
        import torch
        self.torch, self.trainer = torch, trainer
        self.host = [torch.zeros(1).pin_memory() for _ in range(2)]
        self.events = [torch.cuda.Event() for _ in range(2)]
        self.n = 0

    def post(self):
        k = self.n & 1
        self.n += 1
        self.host[k].copy_(self.trainer.last_grad_norm[:1], non_blocking=True)
        self.events[k].record(self.torch.cuda.current_stream(self.trainer.engine.device))
        return k

    def read(self, k):
        self.events[k].synchronize()
        return float(self.host[k][0])

    def now(self):
        """Behind a loss that has just been read back with ``.item()``: the stream is idle, the norm is this step's."""
        return float(self.trainer.last_grad_norm[0])


def train_loop(trainer, train_loader, val_loader, current_step, num_steps, save_interval, log_interval, log, log_dir,
               device_masking=False, word_separator=None, max_epochs=MAX_EPOCHS, deferred_readback=True, reader=None,
               eval_accuracy=False, acc_reader=None):
    """train.py:338-379: validation first, then epochs until ``num_steps``; checkpoint + validation every
    ``save_interval`` steps; every rank logs its LOCAL loss (the reference's rank 0 does).

    ``deferred_readback`` (default): the loss of step i is read back after step i + 1 has been enqueued (``_LossReader``) —
    the same records in the same order as the reference's ``loss.item()`` per step (train.py:395), without its stall. Steps
    that end an interval (checkpoint + validation next) or the run are read back at once, so those happen on exactly the
    weights the reference has there. A step the engine declared invalid (HandoffTimeout; never observed) is found when its
    loss is read — exactly, and at the same step on every rank — and it and the step enqueued behind it (which the device
    left out too: the word is sticky) are run again in order.

    ``eval_accuracy`` (training_params.eval_accuracy; needs a trainer with ``track_accuracy``): every validation record also
    carries val_phoneme_acc / val_phoneme_top5 (``validate_metrics``) and every training record phoneme_acc, the step's top-1
    accuracy at its masked positions, read back beside the loss (``_AccReader``: no new stall). Off: every record is what it
    was."""
    from .engine import HandoffTimeout
    main = world_info()[0] == 0
    window = deque(maxlen=log_interval)
    epoch = 0
    if eval_accuracy and not getattr(trainer, "track_accuracy", False):
        raise ValueError("eval_accuracy needs a trainer built with track_accuracy=True")

    def log_validation():
        if eval_accuracy:
            log(**validate_metrics(trainer, val_loader, device_masking, word_separator), step=current_step, epoch=epoch)
        else:
            log(val_phoneme_loss=validate(trainer, val_loader, device_masking, word_separator), step=current_step, epoch=epoch)

    log_validation()
    train_feeder = _feeder(_source(train_loader, trainer), trainer, word_separator, 0)

    def grant():
        # the training producer may draw up to the next validation point and no further: the validation pass then sees the
        # global masking streams exactly where the reference's single-threaded loop leaves them (train.py:369-373) — on
        # every rank of a data-parallel run alike (each rank draws the global batch's masks, as the reference's ranks do)
        train_feeder.grant(save_interval - current_step % save_interval)

    train_feeder.reset_budget(0)   # permits an earlier loop with this trainer and loader left unused (it stopped mid-interval)
    grant()
    if reader is None:
        reader = _LossReader(trainer.engine.device)
    note = lambda **kw: log(step=current_step, epoch=epoch, **kw)
    # training_params.max_grad_norm: the norm is logged wherever the loss is read back (a step that did not update, the
    # zero-loss fallback, leaves no norm of its own: the record then carries the previous step's)
    norms = _NormReader(trainer) if getattr(trainer, "max_grad_norm", None) is not None else None
    accs = (acc_reader if acc_reader is not None else _AccReader(trainer)) if eval_accuracy else None

    def enqueue(batch):
        """One step and the posts of its read-backs: (loss handle, batch, norm handle, accuracy handle)."""
        loss = trainer.step(batch)
        nk = norms.post() if norms is not None and trainer.last_grad_norm is not None else None
        ak = accs.post() if accs is not None else None
        return (reader.post(loss), batch, nk, ak)

    def rerun(batch):
        loss = _checked(trainer, lambda: trainer.step(batch), note)
        return (loss, (norms.now() if norms is not None and trainer.last_grad_norm is not None else None),
                accs.now() if accs is not None else None)

    def record(loss, grad_norm=None, acc=None):
        nonlocal current_step
        current_step += 1
        window.append(loss)
        rec = {"phoneme_loss": loss, "epoch": epoch, "step": current_step}
        if grad_norm is not None:
            rec["grad_norm"] = grad_norm
        if acc is not None:
            rec["phoneme_acc"] = acc
        if len(window) == log_interval:
            rec["phoneme_loss_avg"] = float(np.mean(window))
        log(**rec)

    def finish(p):
        """Read back and log the pending step p = (handle, batch). True: the engine has declared a step invalid — this one
        (its loss is NaN: it is run again here, checked) or one enqueued behind it that has completed already (this one's
        loss is a number) — and whatever was enqueued behind this step was left out by the device: enqueue it again."""
        import math
        loss = reader.read(p[0])
        grad_norm = norms.read(p[2]) if p[2] is not None else None
        acc = accs.read(p[3]) if p[3] is not None else None
        redo = False
        try:
            trainer.engine.raise_if_failed()     # this step has completed: the word covers it (and may cover a later one)
        except HandoffTimeout as ex:
            note(handoff_timeout=str(ex), retry=1)
            if math.isnan(loss):
                loss, grad_norm, acc = rerun(p[1])
            redo = True
        record(loss, grad_norm, acc)
        return redo

    pending = None                               # a step whose loss has not been read back yet
    while epoch < max_epochs:
        epoch += 1
        for batch in _batches(train_loader, trainer, device_masking, word_separator, 0):
            ahead = current_step + (pending is not None)        # steps enqueued before this one
            try:
                this = enqueue(batch)
            except HandoffTimeout as ex:         # the pending step completed, invalid, before this one was enqueued
                note(handoff_timeout=str(ex), retry=1)
                record(*rerun(pending[1]))
                pending = None
                this = enqueue(batch)
            if pending is not None and finish(pending):
                this = enqueue(batch)
            pending = this
            if not deferred_readback or (ahead + 1) % save_interval == 0 or ahead + 1 >= num_steps:
                finish(pending)                  # (nothing is enqueued behind it: an invalid step is simply run again)
                pending = None
                if current_step % save_interval == 0:
                    save_checkpoint(trainer, current_step, log_dir, epoch, main)
                    log_validation()
                    grant()
                if current_step >= num_steps:
                    return current_step, epoch
        if pending is not None:                  # the epoch's last step
            finish(pending)
            pending = None
    return current_step, epoch


def train(args=None, dataset=None, device=None):
    """Drop-in for ``train.train(args)`` (train.py:133-172): ``args = {'config_path', 'run_name'}``. ``dataset``: rows of
    ``{'phonemes': [...]}``; None loads ``training_params.training_dataset`` with HF ``datasets`` as the reference does."""
    args = args or parse_args()
    # under torchrun / accelerate launch: join the group and take this rank's GPU BEFORE anything touches a device or the
    # run directory (the reference gets both from Accelerator(), train.py:218-221)
    _, _, env_device = init_from_env()
    device = device or env_device
    config, log_dir, resuming = setup_config_and_directories(args, args["config_path"])
    tp, dp = config["training_params"], dict(config["dataset_params"])
    main = world_info()[0] == 0
    print(f"Resuming training from '{log_dir}' with existing config." if resuming else f"Starting new training run in '{log_dir}'.")
    if dataset is None:
        from datasets import load_dataset
        dataset = load_dataset(tp["training_dataset"], split=tp["split"])
    device_masking = bool(tp.get("device_masking", False))
    _, world = world_info()
    # training_params.shard_samples (not in the reference's config.yml): each rank loads and masks only its own samples
    # instead of the whole global batch (build_dataloader(shard=...)); the device-side masking then works under a launcher too
    shard = (world_info()[0], world) if world > 1 and bool(tp.get("shard_samples", False)) else None
    decisions = device_masking and (world == 1 or shard is not None)
    train_loader, val_loader = build_dataloader(dataset, batch_size=int(tp["batch_size"]), device="cuda", dataset_config=dp,
                                                use_token_ids=False, num_workers=int(tp.get("num_workers", 0)),
                                                decisions=decisions, shard=shard)
    trainer, current_step = initialize_model(config, log_dir, resuming, device=device)
    log = _Log(log_dir, main)
    print("Start training...")
    current_step, epoch = train_loop(trainer, train_loader, val_loader, current_step, int(tp["num_steps"]),
                                     int(tp["save_interval"]), int(tp["log_interval"]), log, log_dir,
                                     decisions, dp.get("word_separator"),
                                     eval_accuracy=bool(tp.get("eval_accuracy", False)))
    print(f"Training completed at step {current_step}, epoch {epoch}")
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
    return trainer, current_step, epoch


if __name__ == "__main__":
    train()
