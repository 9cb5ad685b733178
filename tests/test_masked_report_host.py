"""Masked-phoneme evaluation on the CPU (include/plbert.h: plb_masked_report):
 * the instrument — tests/masked_report_ref.py, the numpy restatement of the row / sample / token semantics the GPU tests hold
   the kernels to — is itself held against torch: stable descending sort and torch.topk for the order, float64 logsumexp
   for nll and the log-probabilities, the rank / pred / top-k membership invariants, the NaN row;
 * the new entry point and its three launchers are declared in the headers, exported by the built library and bound;
 * run.validate_metrics and the training_params.eval_accuracy wiring of run.train_loop / run.initialize_model over stand-in
   trainers: the expected records with the key set, byte-for-byte the old records without it."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import c_header
import masked_report_ref as ref
from plbert_amd import _lib

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


# ------------------------------------------------------------------------------------------------------ the instrument
def _rows_case(V, n, seed):
    g = np.random.default_rng(seed)
    z = g.uniform(-80, 80, size=(n, V)).astype(np.float32)
    z[1::3] = g.normal(0, 2, size=z[1::3].shape).astype(np.float32)
    tgt = g.integers(0, V, size=n)
    z[0] = 3.0                                   # a row of equal logits
    if n > 2:                                    # the label ties the maximum at a higher index than another maximum
        z[2] = g.normal(0, 1, size=V).astype(np.float32)
        z[2, 1] = z[2, V - 2] = 9.0
        tgt[2] = V - 2
    if n > 4:
        tgt[3], tgt[4] = 0, V - 1
    if n > 6:                                    # many ties: few distinct values
        z[6] = g.integers(0, 3, size=V).astype(np.float32)
    return z, tgt


@pytest.mark.parametrize("V", [4, 12, 188, 256])
@pytest.mark.parametrize("topk", [0, 1, 5, 8])
def test_instrument_against_torch(V, topk):
    z, tgt = _rows_case(V, 40, seed=V + topk)
    r = ref.rows(z, tgt, topk)
    zt = torch.from_numpy(z).double()
    order = torch.sort(zt, dim=1, descending=True, stable=True).indices      # equal logits keep ascending indices
    k = min(topk, V)
    assert np.array_equal(r.pred, order[:, 0].numpy())
    assert np.array_equal(r.topk_ids[:, :k], order[:, :k].numpy())
    assert bool((r.topk_ids[:, k:] == -1).all()) and bool(np.isneginf(r.topk_logprob[:, k:]).all())
    # rank = the position of the label in that order
    pos = (order == torch.from_numpy(tgt)[:, None]).int().argmax(1).numpy()
    assert np.array_equal(r.rank, pos)
    lse = torch.logsumexp(zt, 1)
    assert np.allclose(r.lse, lse.numpy(), rtol=1e-14, atol=1e-12)
    assert np.allclose(r.nll, (lse - zt[torch.arange(len(tgt)), torch.from_numpy(tgt)]).numpy(), rtol=1e-13, atol=1e-11)
    lsm = torch.log_softmax(zt, 1)
    assert np.allclose(r.topk_logprob[:, :k], torch.gather(lsm, 1, order[:, :k]).numpy(), rtol=1e-13, atol=1e-11)
    # rows without ties: torch.topk agrees as well
    if k:
        distinct = np.array([len(np.unique(row)) == V for row in z])
        tk = torch.topk(zt, k, dim=1).indices.numpy()
        assert distinct.sum() >= 20 and np.array_equal(r.topk_ids[distinct, :k], tk[distinct])
    # invariants
    assert np.array_equal(r.pred == tgt, r.rank == 0)
    member = np.array([tgt[j] in r.topk_ids[j, :k] for j in range(len(tgt))])
    assert np.array_equal(member, r.rank < topk)
    assert r.pred[0] == 0 and r.rank[0] == tgt[0]                          # equal logits: lowest index first
    assert r.rank[2] == 1 and r.pred[2] == 1                                # the tie at a higher index
    assert bool((np.exp(r.topk_logprob[:, :k]).sum(1) <= 1 + 1e-12).all())
    assert bool((np.diff(r.topk_logprob[:, :k], axis=1) <= 0).all())


def test_instrument_nan_row_and_list_longer_than_the_vocabulary():
    z = np.array([[0.5, np.nan, 1.0, 2.0], [1.0, 4.0, 4.0, -np.inf]], np.float32)
    r = ref.rows(z, [2, 3], 5)
    assert r.nan.tolist() == [True, False]
    assert r.pred[0] == -1 and r.rank[0] == 4 and np.isnan(r.nll[0])
    assert bool((r.topk_ids[0] == -1).all()) and bool(np.isnan(r.topk_logprob[0]).all())
    assert r.pred[1] == 1 and r.rank[1] == 3 and np.isposinf(r.nll[1])
    assert r.topk_ids[1].tolist() == [1, 2, 0, 3, -1] and np.isneginf(r.topk_logprob[1, 3:]).all()
    s = ref.samples([0, 1, 2], r.rank, [7.0, 1.0], ref.count_threshold(5, 4))
    assert s.top1.tolist() == [0, 0] and s.topk.tolist() == [0, 1]          # the NaN row (rank V) is never counted correct
    assert s.totals.tolist() == [2, 0, 1, 2]


def test_instrument_samples_and_token_rule():
    off = np.array([0, 5, 5, 22, 23, 23, 63])
    g = np.random.default_rng(5)
    rank = g.integers(0, 9, size=63)
    nll = g.uniform(0, 9, size=63)
    s = ref.samples(off, rank, nll, 5)
    t = torch.from_numpy(nll)
    for b in range(6):
        a, e = off[b], off[b + 1]
        assert abs(s.loss[b] - float(t[a:e].mean())) < 1e-14 if e > a else s.loss[b] == 0.0
        assert s.top1[b] == int((rank[a:e] == 0).sum()) and s.topk[b] == int((rank[a:e] < 5).sum())
    assert s.totals.tolist() == [63, int((rank == 0).sum()), int((rank < 5).sum()), 4]
    assert ref.samples([0, 0, 0], [], [], 5).totals.tolist() == [0, 0, 0, 0]
    assert bool((ref.sample_loss_bound(off, nll)[[1, 4]] == 0).all())
    # token head: tie-inclusive, rows of weight 0 never count
    pmax = np.array([[1.0, 3.0], [2.0, 2.0], [5.0, 0.0], [4.0, 4.5]], np.float32)
    tl = np.array([3.0, 2.0, 5.0, 4.0], np.float32)
    assert ref.token_top1(pmax, tl, np.array([0.1, 0.1, 0.0, 0.1], np.float32)).tolist() == [3, 2]


# --------------------------------------------------------------------------------------------------- header and exports
NEW_LAUNCHERS = ("plb_launch_masked_report_rows", "plb_launch_masked_report_samples", "plb_launch_token_top1")


def test_report_is_declared_exported_and_bound():
    pub, ker = c_header.public(), c_header.kernels()
    assert c_header.c_params(pub, "plb_masked_report") == ["PlbEngine* e", "const int32_t* idx_offsets", "int32_t B", "int32_t topk",
                                                           "const PlbMaskedReport* out", "void* stream"]
    assert [f.name for f in pub.structs["PlbMaskedReport"]] == ["pred", "rank", "nll", "topk_ids", "topk_logprob", "logits",
                                                               "sample_loss", "sample_top1", "sample_topk", "totals",
                                                               "token_totals"]
    assert [f[0] for f in _lib.PlbMaskedReport._fields_] == [f.name for f in pub.structs["PlbMaskedReport"]]
    for name in NEW_LAUNCHERS:
        assert name in ker.protos and name in _lib.INTERNAL, name
    assert c_header.c_params(ker, "plb_launch_masked_report_rows")[:6] == ["const float* logits", "int ldl", "int V",
                                                                           "const int32_t* tgt", "int n", "int topk"]
    assert "plb_masked_report" in _lib.PUBLIC and _lib.PUBLIC["plb_masked_report"][1][4] is _lib.P(_lib.PlbMaskedReport)
    L = _lib.lib()
    readelf = os.path.join(ROCM, "lib", "llvm", "bin", "llvm-readelf")
    out = subprocess.run([readelf, "--dyn-syms", "--wide", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = {ln.split()[7].split("@")[0] for ln in out.splitlines() if len(ln.split()) == 8 and ln.split()[6] != "UND"}
    for name in ("plb_masked_report",) + NEW_LAUNCHERS:
        assert name in exported, name
        fn = getattr(L, name)
        assert (fn.restype, fn.argtypes) == ({**_lib.PUBLIC, **_lib.INTERNAL}[name][0], {**_lib.PUBLIC, **_lib.INTERNAL}[name][1])


def test_host_api_carries_the_report():
    import inspect

    from plbert_amd.engine import HipEngine
    from plbert_amd.model import MultiTaskModel, PhonemeOnlyModel
    from plbert_amd.train import PLBertTrainer
    sig = inspect.signature(HipEngine.masked_report).parameters
    assert sig["topk"].default == 5 and sig["want"].default == ("totals",)
    assert set(HipEngine.REPORT_OUTPUTS) == {f[0] for f in _lib.PlbMaskedReport._fields_}
    assert inspect.signature(PLBertTrainer.__init__).parameters["track_accuracy"].default is False
    assert inspect.signature(PLBertTrainer.evaluate).parameters["topk"].default == 5
    for cls in (PhonemeOnlyModel, MultiTaskModel):
        p = inspect.signature(cls.fill_mask).parameters
        assert list(p)[1:] == ["phonemes", "positions", "attention_mask", "topk"] and p["topk"].default == 5


# -------------------------------------------------------------------------------------------------------------- records
class _Loss(float):
    def item(self):
        return float(self)


class _Batch:
    def __init__(self, i, totals):
        self.i, self.offsets, self.totals = i, ("offsets", i), totals


class _Engine:
    device = "sim"

    def __init__(self):
        self.asked, self.last = [], None

    def raise_if_failed(self):
        pass

    def masked_report(self, offsets, topk=5, want=("totals",), out=None):
        assert offsets == ("offsets", self.last.i), "the report must follow the batch's own loss call"
        self.asked.append((self.last.i, topk, tuple(want)))
        return {"totals": torch.tensor(self.last.totals, dtype=torch.int32)}


class _Trainer:
    def __init__(self, track):
        self.engine, self.track_accuracy, self.last_accuracy, self.steps = _Engine(), track, None, []

    def loss_only(self, b):
        self.engine.last = b
        return _Loss(1.0 + b.i)

    def step(self, b):
        self.steps.append(b.i)
        if self.track_accuracy:
            self.last_accuracy = list(b.totals)
        return _Loss(10.0 + b.i)


VAL = [[10, 5, 8, 2], [0, 0, 0, 0], [30, 3, 12, 4]]
TRAIN = [[8, 2, 4, 2], [0, 0, 0, 0], [5, 5, 5, 1], [4, 1, 2, 1]]


def _patch(monkeypatch):
    from plbert_amd import run
    monkeypatch.setattr(run, "_batches", lambda loader, *a, **k: iter(loader))
    monkeypatch.setattr(run, "_source", lambda loader, trainer: loader)
    monkeypatch.setattr(run, "save_checkpoint", lambda *a, **k: None)

    class Budget:
        def grant(self, n): pass
        def reset_budget(self, n=0): pass

    monkeypatch.setattr(run, "_feeder", lambda *a, **k: Budget())
    return run


def test_validate_metrics_is_validate_plus_micro_averages(monkeypatch):
    run = _patch(monkeypatch)
    val = [_Batch(i, t) for i, t in enumerate(VAL)]
    tr = _Trainer(False)
    m = run.validate_metrics(tr, val)
    assert list(m) == ["val_phoneme_loss", "val_phoneme_acc", "val_phoneme_top5"]
    assert m["val_phoneme_loss"] == run.validate(_Trainer(False), val) == 2.0          # validate's value and type
    assert m["val_phoneme_acc"] == 8 / 40 and m["val_phoneme_top5"] == 20 / 40        # summed correct over summed rows
    assert tr.engine.asked == [(0, 5, ("totals",)), (1, 5, ("totals",)), (2, 5, ("totals",))]
    m3 = run.validate_metrics(_Trainer(False), val, topk=3)
    assert list(m3) == ["val_phoneme_loss", "val_phoneme_acc", "val_phoneme_top3"]
    empty = run.validate_metrics(_Trainer(False), [_Batch(0, [0, 0, 0, 0])])
    assert empty == {"val_phoneme_loss": 1.0, "val_phoneme_acc": 0.0, "val_phoneme_top5": 0.0}
    assert run.validate_metrics(_Trainer(False), []) == {"val_phoneme_loss": 0.0, "val_phoneme_acc": 0.0, "val_phoneme_top5": 0.0}


class _Reader:
    def post(self, loss): return loss
    def read(self, h): return float(h)


class _Accs:
    def __init__(self, trainer): self.trainer = trainer
    def post(self): return list(self.trainer.last_accuracy)
    def read(self, h): return h[1] / h[0] if h[0] else 0.0
    def now(self): return self.read(self.trainer.last_accuracy)


def _loop(run, trainer, **kw):
    recs = []
    val = [_Batch(i, t) for i, t in enumerate(VAL)]
    train = [_Batch(i, t) for i, t in enumerate(TRAIN)]
    step, _ = run.train_loop(trainer, train, val, 0, 4, 2, 2, lambda **r: recs.append(json.dumps(r)), "unused", reader=_Reader(),
                             **kw)
    assert step == 4 and trainer.steps == [0, 1, 2, 3]
    return recs


@pytest.mark.parametrize("deferred", [True, False])
def test_eval_accuracy_records(monkeypatch, deferred):
    run = _patch(monkeypatch)
    # the key absent: byte for byte the records of today
    old = _loop(run, _Trainer(False), deferred_readback=deferred)
    assert old == [
        '{"val_phoneme_loss": 2.0, "step": 0, "epoch": 0}',
        '{"phoneme_loss": 10.0, "epoch": 1, "step": 1}',
        '{"phoneme_loss": 11.0, "epoch": 1, "step": 2, "phoneme_loss_avg": 10.5}',
        '{"val_phoneme_loss": 2.0, "step": 2, "epoch": 1}',
        '{"phoneme_loss": 12.0, "epoch": 1, "step": 3, "phoneme_loss_avg": 11.5}',
        '{"phoneme_loss": 13.0, "epoch": 1, "step": 4, "phoneme_loss_avg": 12.5}',
        '{"val_phoneme_loss": 2.0, "step": 4, "epoch": 1}']
    assert _loop(run, _Trainer(True), deferred_readback=deferred) == old      # a tracking trainer alone changes no record
    tr = _Trainer(True)
    new = [json.loads(r) for r in _loop(run, tr, deferred_readback=deferred, eval_accuracy=True, acc_reader=_Accs(tr))]
    vals = [r for r in new if "val_phoneme_loss" in r]
    assert vals == [{"val_phoneme_loss": 2.0, "val_phoneme_acc": 0.2, "val_phoneme_top5": 0.5, "step": s, "epoch": e}
                    for s, e in ((0, 0), (2, 1), (4, 1))]
    steps = [r for r in new if "phoneme_loss" in r]
    old_steps = [r for r in map(json.loads, old) if "phoneme_loss" in r]
    assert [r["phoneme_acc"] for r in steps] == [0.25, 0.0, 1.0, 0.25] and [r["step"] for r in steps] == [1, 2, 3, 4]
    assert [{k: v for k, v in r.items() if k != "phoneme_acc"} for r in steps] == old_steps
    with pytest.raises(ValueError, match="track_accuracy"):
        _loop(run, _Trainer(False), eval_accuracy=True)


@pytest.mark.parametrize("setting", [None, True, False])
def test_run_hands_eval_accuracy_to_the_trainer(monkeypatch, tmp_path, setting):
    from plbert_amd import run, train
    got = {}

    class FakeTrainer:
        def __init__(self, cfg, **kw):
            got.update(kw)

    monkeypatch.setattr(train, "PLBertTrainer", FakeTrainer)
    monkeypatch.setattr(run, "albert_config_from_yaml", lambda config, n: None)
    tp = {"batch_size": 4, "learning_rate": 1e-4}
    if setting is not None:
        tp["eval_accuracy"] = setting
    run.initialize_model({"training_params": tp, "dataset_params": {"max_seq_length": 128}, "model_params": {}}, str(tmp_path),
                         resuming=False)
    assert got["track_accuracy"] is bool(setting)
