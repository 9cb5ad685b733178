"""plb_token_report end to end (-m gpu): the token head's predictions from the hidden state a call left behind, no logits stored.

 A. After every qualifying call form the ids / target_pos / totals equal the instrument (tests/token_report_ref.py) applied to
    the report's OWN logits; those logits equal plb_forward's token_logits at the same positions within the GEMM family's
    bound (K + 3) 2^-23 (sum |a||b| + |bias|), formed from the forward's hidden output and the bf16-rounded weights, and the
    fixture's reference token_logits within the 3e-2 test_gpu_model_api.py / test_gpu_dual_head.py use. (An fp8 LOSS call is
    held to the instrument only: no second call reproduces its hidden state — every fp8 call updates the delayed scales; the
    fp8 FORWARD is held to its own hidden and token_logits outputs.)
 B. These are the call's numbers: minus the mean over samples of the mean over valid positions of target_logprob is the token
    term of loss_parts within the bound stated at _token_loss_bound.
 C. totals against plb_masked_report's token_totals: same rows, exact <= tie-inclusive, equal where no row ties.
 D. By construction: a bias spike leads every row with log-probability ~0; a zero head gives ids 0..k-1 at -log(num_tokens).
 E. Every refusal fails with its text and launches nothing.
 F. Nothing changes: the training sequence with and without the report is the same bits, plb_masked_report too, a live
    plb_encode stash stays live, a step that does not ask launches what it launched.
 G. The host API: predict_tokens against torch.topk of the model's own token logits, evaluate, validate_metrics.

Models: the small_h128_multitask / small_h128_dualloss fixtures (H 128, L 2, 3 x 40, lengths 40 / 33 / 7, num_tokens 96) on a
training and an inference-only engine; a 768-wide two-layer model with num_tokens 1000 at B 3, S 256, lengths 256 / 130 / 40,
where a packing plan (640 rows), plb_set_packed_dual and fp8 mode exist.
Observed on an MI355X (pytest -s): logits against the float64 product of the forward's hidden output at most 0.0012 of the
GEMM bound (0 against plb_forward's token_logits: the same K loop); token loss 5.5195646 against 5.5195644 from the report
(bound 3.5e-5) on the small model, 7.1059055 against 7.1059049 (bound 5.6e-5) on the wide one."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import golden_cfg, load_golden
import token_report_ref as ref
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import HipEngine, packing_plan
from plbert_amd.train import PLBertTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U32 = ref.U32
ALL = ("topk_ids", "topk_logprob", "lse", "target_logprob", "target_pos", "logits", "totals")
WIDE_LENS = [256, 130, 40]


@pytest.fixture(autouse=True)
def _prune_hook_back_to_the_environment():
    yield
    _lib.lib().plb_set_prune_last(-1)


# ------------------------------------------------------------------------------------------------------------ inputs
def _small_case():
    g = load_golden("small_h128_dualloss")
    idx = [list(map(int, x)) for x in g["index"]]
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    return g, dict(masked=g["masked"], labels=g["labels"], lens=g["lengths"].astype(np.int32), off=off, flat=flat,
                   n=int(off[-1]), tok=g["token_ids"])


def _small_engine(g, train=True):
    _, pcfg, sd = golden_cfg(g)
    B, S = g["labels"].shape
    eng = HipEngine(pcfg, int(g["num_phonemes"]), int(g["num_tokens"]), max_batch=B, max_seq=S, train=train)
    eng.load_state_dict(sd)
    return eng


@functools.lru_cache(maxsize=None)
def _wide_model():
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  max_position_embeddings=512, num_hidden_layers=2)
    return cfg, plbert_amd.deterministic_state_dict(cfg, 188, 1000, seed=5)


@functools.lru_cache(maxsize=None)
def _wide_case(seed=7):
    B, S = 3, 256
    labels, masked, _, idx = plbert_amd.synthetic_batch(B, S, seed=seed)
    idx = [[i for i in ix if i < n] or [0] for ix, n in zip(idx, WIDE_LENS)]
    for b, n in enumerate(WIDE_LENS):
        labels[b, n:] = 0
        masked[b, n:] = 0
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    tok = np.random.default_rng(seed).integers(0, 1000, size=(B, S)).astype(np.int64)
    return dict(masked=masked, labels=labels, lens=np.asarray(WIDE_LENS, np.int32), off=off, flat=flat, n=int(off[-1]), tok=tok)


def _wide_engine(train=True):
    cfg, sd = _wide_model()
    eng = HipEngine(cfg, 188, 1000, max_batch=3, max_seq=256, train=train)
    eng.load_state_dict(sd)
    return eng


def _args(c):
    return (c["masked"], c["labels"], c["lens"], c["off"], c["flat"], c["n"])


def _np(rep):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in rep.items()}


def _same_bits(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def _valid(c):
    B, S = c["masked"].shape
    return (np.arange(S)[None, :] < c["lens"][:, None]).reshape(-1)


# ------------------------------------------------------------------------------------------------------------ checks
def _check_own(rep, c, NT, topk=5):
    """A: the report on every position against the instrument applied to the report's own logits."""
    valid = _valid(c)
    n = valid.size
    z = rep["logits"]
    assert z.shape == (n, NT) and bool(np.isfinite(z).all()) and bool((z[~valid] == 0).all())
    rows = np.where(valid, 0, -1)
    want = ref.report(z, c["tok"].reshape(-1), topk, rows)
    assert np.array_equal(rep["topk_ids"], want.topk_ids) and np.array_equal(rep["target_pos"], want.target_pos)
    assert np.array_equal(rep["totals"], want.totals) and want.totals[0] == int(valid.sum())
    ns = ref.strips(n, NT)
    for got, w, zz in ((rep["lse"], want.lse, 0.0), (rep["target_logprob"], want.target_logprob, want.target_logprob + want.lse)):
        assert np.isnan(got[~valid]).all()
        b = ref.logprob_bound(want.lse[valid], np.asarray(zz)[valid] if np.ndim(zz) else 0.0, w[valid], NT, ns)
        assert bool((np.abs(got[valid].astype(np.float64) - w[valid]) <= b).all())
    lp = rep["topk_logprob"].astype(np.float64)
    assert np.isneginf(lp[~valid]).all() and bool((rep["topk_ids"][~valid] == -1).all())
    b = ref.logprob_bound(want.lse[valid, None], want.topk_logprob[valid] + want.lse[valid, None], want.topk_logprob[valid], NT, ns)
    assert bool((np.abs(lp[valid] - want.topk_logprob[valid]) <= b).all())
    return want


def _check_against_forward(eng, rep, c, NT, hid=None, tk=None, plan=None):
    """A: the report's logits within the GEMM bound of the float64 product of the forward's hidden output (the bf16 rows,
    exactly) and the bf16-rounded weights, and within the same bound of plb_forward's token_logits of the same input. A call
    that ran token-packed is held to the hidden output of the PACKED forward and to the float64 product alone: token_logits
    make a forward run padded (include/plbert.h), and the padded run's hidden rows are other bf16 roundings of the same
    values (tile boundaries of the fused LayerNorm fall elsewhere), so no token_logits of that hidden state exist."""
    if hid is None and plan is not None:
        hid, _, _ = eng.forward(c["masked"], c["lens"], want_hidden=True, want_phoneme=False, packing=plan)
        assert eng.last_call_rows()[0] == plan.rows
    elif hid is None:
        hid, _, tk = eng.forward(c["masked"], c["lens"], want_hidden=True, want_phoneme=False, want_token=True)
    valid = _valid(c)
    H = hid.shape[-1]
    W = eng.view("token_predictor.weight").to(torch.bfloat16).double().cpu().numpy()
    bias = eng.view("token_predictor.bias").double().cpu().numpy()
    A = hid.double().cpu().numpy().reshape(-1, H)[valid]
    bound = (H + 3) * 2.0 ** -23 * (np.abs(A) @ np.abs(W).T + np.abs(bias))
    err = np.abs(rep["logits"][valid].astype(np.float64) - (A @ W.T + bias))
    assert bool((err <= bound).all()), float((err / bound).max())
    worst = float((err / bound).max())
    if tk is not None:
        err = np.abs(rep["logits"][valid].astype(np.float64) - tk.double().cpu().numpy().reshape(-1, NT)[valid])
        assert bool((err <= bound).all()), float((err / bound).max())
        worst = max(worst, float((err / bound).max()))
    return worst


def _report_all(eng, c, topk=5, want=ALL):
    return _np(eng.token_report(None, c["tok"], topk=topk, want=want))


# ------------------------------------------------------------------------------------- A. every qualifying call form
@pytest.mark.parametrize("train", [True, False], ids=["training", "inference"])
def test_small_forward_and_the_reference_logits(train):
    g = load_golden("small_h128_multitask")
    _, c = _small_case()
    NT = int(g["num_tokens"])
    c = dict(c, masked=g["masked"], tok=c["tok"] % NT)     # (the other fixture's targets, folded into this head's classes)
    eng = _small_engine(g, train)
    hid, _, tk = eng.forward(c["masked"], c["lens"], want_hidden=True, want_phoneme=False, want_token=True)
    rep = _report_all(eng, c, topk=8)
    _check_own(rep, c, NT, topk=8)
    _check_against_forward(eng, rep, c, NT, hid, tk)
    valid = _valid(c)
    assert float(np.abs(rep["logits"][valid] - g["token_logits"].reshape(-1, NT)[valid]).max()) < 3e-2
    # a forward that outputs nothing leaves the same state; the CSR form reports the same rows
    eng.forward(c["masked"], c["lens"], want_hidden=False, want_phoneme=False, want_token=False)
    assert _same_bits(rep, _report_all(eng, c, topk=8))
    off, flat = plbert_amd.masked_indices_to_csr([list(range(int(n))) for n in c["lens"]])
    csr = _np(eng.token_report((off, flat), c["tok"], topk=8, want=ALL))
    for k in ("topk_ids", "topk_logprob", "lse", "target_logprob", "target_pos", "logits"):
        assert np.array_equal(csr[k].view(np.uint32), rep[k][valid].view(np.uint32)), k
    assert np.array_equal(csr["totals"], rep["totals"])
    # only what is asked for: topk 0, no targets
    r0 = _np(eng.token_report(None, None, topk=0, want=("lse", "topk_ids")))
    assert r0["topk_ids"].shape == (valid.size, 0) and np.array_equal(r0["lse"].view(np.uint32), rep["lse"].view(np.uint32))


@pytest.mark.parametrize("form", ["loss_only_dual", "training_dual", "encode"])
def test_small_call_forms(form):
    g, c = _small_case()
    eng = _small_engine(g)
    NT = int(g["num_tokens"])
    if form == "encode":
        eng.encode(c["masked"], c["lens"])
    else:
        (eng.loss_fwd if form == "loss_only_dual" else eng.loss_fwd_bwd)(*_args(c), token_ids=c["tok"])
    rep = _report_all(eng, c)
    _check_own(rep, c, NT)
    _check_against_forward(eng, rep, c, NT)
    assert _same_bits(rep, _report_all(_forwarded(_small_engine(g), c), c))        # the same hidden bits whatever call left them


def _forwarded(eng, c, **kw):
    eng.forward(c["masked"], c["lens"], want_hidden=False, want_phoneme=False, want_token=False, **kw)
    return eng


@pytest.mark.parametrize("form", ["forward", "packed_forward", "training_dual_padded", "training_dual_packed", "loss_only_packed",
                                  "inference_packed_forward"])
def test_wide_call_forms(form):
    c = _wide_case()
    eng = _wide_engine(train=not form.startswith("inference"))
    plan = packing_plan(WIDE_LENS, 256).to(DEV, non_blocking=False) if "packed" in form else None
    assert plan is None or (plan.packed and plan.rows == 640)
    if "forward" in form:
        _forwarded(eng, c, packing=plan)
    else:
        eng.set_packed_dual("packed" in form)
        (eng.loss_fwd if form.startswith("loss_only") else eng.loss_fwd_bwd)(*_args(c), token_ids=c["tok"], packing=plan)
    assert (eng.last_call_rows()[0] == 640) == ("packed" in form)
    rep = _report_all(eng, c)
    want = _check_own(rep, c, 1000)
    print(f"\n{form}: logits against plb_forward, worst fraction of the GEMM bound", _check_against_forward(eng, rep, c, 1000, plan=plan))
    # C: the exact count against the tie-inclusive one of plb_masked_report (random weights: no row ties, so they agree)
    if "dual" in form or form == "loss_only_packed":
        tt = eng.masked_report(c["off"], want=("token_totals",))["token_totals"].cpu().tolist()
        top2 = np.sort(rep["logits"][_valid(c)], 1)[:, -2:]
        assert bool((top2[:, 1] > top2[:, 0]).all())
        assert rep["totals"][0] == tt[0] and rep["totals"][1] == tt[1] == int((want.target_pos == 0).sum())


def test_fp8_forward_and_fp8_training_call():
    c = _wide_case()
    eng = _wide_engine()
    eng.set_fp8(True)
    for step in (1, 2):                              # the calibration calls
        eng.loss_fwd_bwd(*_args(c), token_ids=c["tok"])
        eng.adamw_step(step, lr=1e-4)
    eng.loss_fwd_bwd(*_args(c), token_ids=c["tok"])
    assert eng.fp8_state() == (True, True)
    _check_own(_report_all(eng, c), c, 1000)
    hid, _, tk = eng.forward(c["masked"], c["lens"], want_hidden=True, want_phoneme=False, want_token=True)
    rep = _report_all(eng, c)
    _check_own(rep, c, 1000)
    _check_against_forward(eng, rep, c, 1000, hid, tk)


# -------------------------------------------------------------------------------------- B. the call's own numbers
def _token_loss_bound(rep, c, NT):
    """The call's token term is sum over the valid rows of fl(w_r * (lse_r - z_t)), w_r = 1 / (B * len_b), added by sum_rows in
    chains of ceil(rows / 256) terms, 6 butterfly steps and 3 wave additions; here the same rows are averaged in float64 from
    the report's target_logprob. What differs: the summation (depth + 2 roundings — w and the product — of the absolute row
    sum), and per row the two evaluations of lse - z_t, each within logprob_bound of the exact value (the call merges its
    256-column tiles' (max, sum) pairs, chains of 64 terms per lane: no deeper than the report's single strip)."""
    valid = _valid(c)
    B, S = c["masked"].shape
    w = np.repeat(1.0 / (B * c["lens"].astype(np.float64)), S)[valid]
    tlp = rep["target_logprob"][valid].astype(np.float64)
    lse = rep["lse"][valid].astype(np.float64)
    depth = -(-valid.size // 256) + 9 + 2
    rows = 2 * ref.logprob_bound(lse, tlp + lse, tlp, NT, 1)
    return depth * U32 * float(np.abs(w * tlp).sum()) + float((w * rows).sum()), -float((w * tlp).sum())


@pytest.mark.parametrize("wide", [False, True], ids=["small", "wide"])
def test_target_logprob_is_the_calls_token_loss(wide):
    if wide:
        c, eng, NT = _wide_case(), _wide_engine(train=False), 1000
    else:
        g, c = _small_case()
        eng, NT = _small_engine(g, train=False), int(g["num_tokens"])
    eng.loss_fwd(*_args(c), token_ids=c["tok"])
    torch.cuda.synchronize()
    token_loss = float(eng.loss_parts[1].item())
    bound, mine = _token_loss_bound(_report_all(eng, c), c, NT)
    print(f"\ntoken loss {token_loss}, from the report {mine}, bound {bound}")
    assert abs(mine - token_loss) <= bound, (mine, token_loss, bound)
    assert bound < 1e-4 * abs(token_loss)


# ----------------------------------------------------------------------------------------------- D. by construction
def test_bias_spike_and_zero_head():
    g, c = _small_case()
    NT = int(g["num_tokens"])
    eng = _small_engine(g)
    valid = _valid(c)
    spike = 17
    tok = np.full(c["masked"].shape, (spike + 1) % NT, np.int64)
    subset = valid.reshape(tok.shape) & (np.random.default_rng(3).random(tok.shape) < 0.3)
    subset[0, 0] = True
    tok[subset] = spike
    tok[~valid.reshape(tok.shape)] = spike             # pad positions carry the "correct" class: they must not count
    eng.view("token_predictor.bias")[spike] += 30.0
    eng.sync_weights()
    eng.loss_fwd_bwd(*_args(c), token_ids=tok)
    rep = _np(eng.token_report(None, tok, want=ALL))
    assert bool((rep["topk_ids"][valid, 0] == spike).all())
    lse, lp0 = rep["lse"][valid].astype(np.float64), rep["topk_logprob"][valid, 0].astype(np.float64)
    assert bool((np.abs(lp0) <= ref.logprob_bound(lse, lse, 0.0, NT, 1) + NT * np.exp(-20.0)).all())   # (the others: logits ~ +-1)
    assert rep["totals"].tolist()[:2] == [int(valid.sum()), int(subset.sum())] and rep["totals"][2] >= rep["totals"][1]
    tt = eng.masked_report(c["off"], want=("token_totals",))["token_totals"].cpu().tolist()
    assert tt == [int(valid.sum()), int(subset.sum())]
    # a zero head: ids 0 .. k-1, every log-probability -log(num_tokens); the exact rule counts class 0 only, the tie-inclusive all
    eng.view("token_predictor.weight").zero_()
    eng.view("token_predictor.bias").zero_()
    eng.sync_weights()
    eng.loss_fwd(*_args(c), token_ids=c["tok"])
    rep = _np(eng.token_report(None, c["tok"], topk=8, want=ALL))
    assert bool((rep["topk_ids"][valid] == np.arange(8)).all())
    assert bool((np.abs(rep["topk_logprob"][valid].astype(np.float64) + np.log(NT)) <= ref.logprob_bound(np.log(NT), 0.0, np.log(NT), NT, 1)).all())
    t = c["tok"].reshape(-1)[valid]
    tt = eng.masked_report(c["off"], want=("token_totals",))["token_totals"].cpu().tolist()
    assert rep["totals"].tolist() == [int(valid.sum()), int((t == 0).sum()), int((t < 8).sum())]
    assert rep["totals"][1] <= tt[1] == int(valid.sum())


# ------------------------------------------------------------------------------------------------------ E. refusals
def _raw(eng, c, n=None, B=None, S=None, topk=5, lens=True, tok=True, packing=None, csr=None, **ptrs):
    rep = _lib.PlbTokenReport()
    for k, v in ptrs.items():
        setattr(rep, k, v.data_ptr())
    b, s = c["masked"].shape
    B, S = b if B is None else B, s if S is None else S
    keep = [eng._dev_i32(c["lens"]), eng._dev_i64(c["tok"])]
    offs = flat = None
    if csr is not None:
        offs, flat = eng._dev_i32(csr[0]), eng._dev_i32(csr[1])
    rc = eng.L.plb_token_report(eng.handle, keep[0].data_ptr() if lens else None, None if offs is None else offs.data_ptr(),
                                None if flat is None else flat.data_ptr(), b * s if n is None else n, B, S,
                                None if packing is None else C.byref(packing), keep[1].data_ptr() if tok else None, topk,
                                C.byref(rep), eng._stream())
    return rc, eng.L.plb_last_error().decode()


def test_refusals_launch_nothing():
    g, c = _small_case()
    tot = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    ids = torch.full((120, 8), -7, dtype=torch.int32, device=DEV)
    tlp = torch.full((120,), 7.0, device=DEV)
    P = "plb_token_report: "
    _lib.profile_enable(True)
    try:
        eng = _small_engine(g)
        assert _raw(eng, c, totals=tot) == (1, P + "engine not bound")
        with pytest.raises(RuntimeError, match="no call has run the encoder"):
            eng.token_report()
        eng._bind()
        eng.sync_weights()
        torch.cuda.synchronize()
        _lib.profile_read()
        rc, text = _raw(eng, c, totals=tot)
        assert rc == 1 and text.startswith(P + "no final hidden state to report on: plb_sync_weights refreshed")
        # no token head
        g0 = load_golden("small_h128")
        e0 = _small_engine(g0)
        e0.forward(c["masked"], c["lens"], want_phoneme=False)
        torch.cuda.synchronize()
        _lib.profile_read()
        assert _raw(e0, c, topk_ids=ids) == (1, P + "the engine has no token head (num_tokens = 0)")
        with pytest.raises(RuntimeError, match="no token head"):
            e0.token_report()
        # a call without anything to run, then a real one
        B = len(c["lens"])
        eng.loss_fwd(c["masked"], c["labels"], c["lens"], np.zeros(B + 1, np.int32), np.zeros(0, np.int32), 0)
        torch.cuda.synchronize()
        _lib.profile_read()
        rc, text = _raw(eng, c, totals=tot)
        assert rc == 1 and "it did not run the encoder" in text
        eng.loss_fwd_bwd(*_args(c), token_ids=c["tok"])
        torch.cuda.synchronize()
        _lib.profile_read()
        assert _raw(eng, c, B=4, totals=tot) == (1, P + "batch 4 x seq 40 differs from the reported call's 3 x 40")
        assert _raw(eng, c, S=39, n=117, totals=tot) == (1, P + "batch 3 x seq 39 differs from the reported call's 3 x 40")
        for topk in (9, -1):
            assert _raw(eng, c, topk=topk, topk_ids=ids) == (1, P + f"topk {topk} outside [0, 8]")
        assert _raw(eng, c, tok=False, totals=tot) == (1, P + "totals wanted but token_ids is null")
        assert _raw(eng, c, tok=False, target_logprob=tlp) == (1, P + "a target output wanted but token_ids is null")
        assert _raw(eng, c, n=-1, topk_ids=ids)[1] == P + "n -1 outside [0, 120], the call's positions"
        assert _raw(eng, c, n=121, csr=(c["off"], c["flat"]), topk_ids=ids)[1] == P + "n 121 outside [0, 120], the call's positions"
        assert _raw(eng, c, n=119, topk_ids=ids)[1] == P + "idx_offsets is null (every position), so n must be B*S = 120, not 119"
        plan = packing_plan(WIDE_LENS, 256).to(DEV, non_blocking=False)
        rc, text = _raw(eng, c, packing=plan.c_struct(DEV), totals=tot)
        assert rc == 1 and text == P + "packing plan of 640 rows exceeds the reported call's 128"
        with pytest.raises(ValueError, match="unknown output"):
            eng.token_report(want=("accuracy",))
        torch.cuda.synchronize()
        assert _lib.profile_read() == {}                                  # nothing was launched
        assert bool((tot == -7).all()) and bool((ids == -7).all()) and bool((tlp == 7.0).all())
        # n == 0 is no refusal: zeros in totals, no row output, no kernel
        assert _raw(eng, c, n=0, csr=(np.zeros(B + 1, np.int32), np.zeros(1, np.int32)), totals=tot, topk_ids=ids)[0] == 0
        torch.cuda.synchronize()
        assert tot.tolist() == [0, 0, 0] and bool((ids == -7).all()) and _lib.profile_read() == {}
        # and the report is still there: one strip launch under gemm_nt_ce, prepare + merge + totals under token_ce
        tot.fill_(-7)
        assert _raw(eng, c, totals=tot)[0] == 0
        torch.cuda.synchronize()
        prof = _lib.profile_read()
        assert tot.tolist()[0] == int(c["lens"].sum()) and {k: v["launches"] for k, v in prof.items()} == {"gemm_nt_ce": 1, "token_ce": 2}
        # the weights moved
        eng.adamw_step(1, lr=1e-3)
        rc, text = _raw(eng, c, totals=tot)
        assert rc == 1 and text.startswith(P + "no final hidden state to report on: plb_adamw_step moved the weights since")
        with pytest.raises(RuntimeError, match="moved the weights"):
            eng.token_report(None, c["tok"], want=("totals",))
    finally:
        _lib.profile_enable(False)


def test_a_pruned_call_and_another_plan_are_refused():
    c = _wide_case()
    eng = _wide_engine()
    _lib.lib().plb_set_prune_last(1)
    eng.loss_fwd_bwd(*_args(c))                          # phoneme-only, <= 256 masked rows of 768: pruned
    rows, of = eng.last_application_rows()
    assert rows < of
    with pytest.raises(RuntimeError, match="pruned its last application"):
        eng.token_report()
    _lib.lib().plb_set_prune_last(0)
    eng.loss_fwd_bwd(*_args(c))                          # the same call unpruned leaves one
    rep = _report_all(eng, c)
    _check_own(rep, c, 1000)
    # a packed call must be reported with its plan
    plan = packing_plan(WIDE_LENS, 256).to(DEV, non_blocking=False)
    _forwarded(eng, c, packing=plan)
    rc, text = _raw(eng, c, topk_ids=torch.zeros((768, 5), dtype=torch.int32, device=DEV))
    assert rc == 1 and "ran token-packed (640 rows, 640 used): its lengths and packing plan are needed" in text
    other = packing_plan([256, 256, 40], 256).to(DEV, non_blocking=False)
    rc, text = _raw(eng, c, packing=other.c_struct(DEV), topk_ids=torch.zeros((768, 5), dtype=torch.int32, device=DEV))
    assert rc == 1 and "packing plan differs from the reported call's" in text
    _check_own(_report_all(eng, c), c, 1000)             # with its own plan it reports


# ------------------------------------------------------------------------------------------- F. nothing changes
def test_the_training_sequence_is_the_same_bits_with_and_without_the_report():
    g, c = _small_case()
    a, b = _small_engine(g), _small_engine(g)
    la = float(a.loss_fwd_bwd(*_args(c), token_ids=c["tok"]).item())
    mr_before = _np(a.masked_report(c["off"], want=("nll", "rank", "totals", "token_totals", "logits")))
    rep = _report_all(a, c)
    assert _same_bits(mr_before, _np(a.masked_report(c["off"], want=("nll", "rank", "totals", "token_totals", "logits"))))
    assert a.poll_status()["ln_exchange_timeouts"] == 0
    lb = float(b.loss_fwd_bwd(*_args(c), token_ids=c["tok"]).item())
    assert np.float32(la).view(np.uint32) == np.float32(lb).view(np.uint32) and torch.equal(a.grads, b.grads)
    a.adamw_step(1, lr=1e-3)
    b.adamw_step(1, lr=1e-3)
    assert torch.equal(a.params, b.params) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    la, lb = float(a.loss_fwd_bwd(*_args(c), token_ids=c["tok"]).item()), float(b.loss_fwd_bwd(*_args(c), token_ids=c["tok"]).item())
    assert np.float32(la).view(np.uint32) == np.float32(lb).view(np.uint32) and torch.equal(a.grads, b.grads)
    assert not _same_bits(rep, _report_all(a, c))        # (and the report follows the weights)
    assert _same_bits(_report_all(a, c), _report_all(b, c))


def test_a_live_encode_stash_survives_a_report():
    g, c = _small_case()
    eng = _small_engine(g)
    hid = eng.encode(c["masked"], c["lens"])
    rep = _report_all(eng, c)
    eng.encode_bwd(torch.ones_like(hid))                 # the stash was still live
    torch.cuda.synchronize()
    assert float(eng.grads[: eng.layout["phoneme_predictor.weight"][0]].abs().sum()) > 0
    assert _same_bits(rep, _report_all(eng, c))          # the backward wrote no hidden state and moved no weight


def _small_cfg():
    return plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)


def _dual_batch(tr, seed=41, lengths=(32, 19, 26, 11), S=32):
    labels, masked, _, idx = plbert_amd.synthetic_batch(len(lengths), S, seed=seed)
    out = []
    for b, n in enumerate(lengths):
        out.append([i for i in idx[b] if i < n] or [n // 2])
        labels[b, n:] = 0
        masked[b, n:] = 0
    tok = np.random.default_rng(seed).integers(0, 300, size=labels.shape).astype(np.int64)
    return tr.stage_batch(labels, masked, np.asarray(lengths, np.int32), out, token_ids=tok)


def _trainer():
    sd = plbert_amd.deterministic_state_dict(_small_cfg(), 188, 300, seed=8)
    return PLBertTrainer(_small_cfg(), 188, num_tokens=300, max_batch=4, max_seq=32, lr=1e-3, state_dict=sd)


def test_a_step_that_does_not_ask_launches_what_it_launched():
    def counts(tr):
        batch = _dual_batch(tr)
        tr.step(batch)
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        try:
            _lib.profile_read()
            tr.step(batch)
            torch.cuda.synchronize()
            return {k: v["launches"] for k, v in _lib.profile_read().items()}
        finally:
            _lib.profile_enable(False)

    base = counts(_trainer())
    used = _trainer()
    ev = used.evaluate(_dual_batch(used))                # the new entry point once, then the default step again
    assert counts(used) == base, base
    # G: evaluate on a dual-head batch adds token_exact beside token_totals
    assert sorted(ev) == ["loss", "sample_loss", "sample_top1", "sample_topk", "token_exact", "token_totals", "totals"]
    te, tt = ev["token_exact"].cpu().tolist(), ev["token_totals"].cpu().tolist()
    assert te[0] == tt[0] == 32 + 19 + 26 + 11 and 0 <= te[1] <= tt[1] and te[1] <= te[2] <= te[0]


# ------------------------------------------------------------------------------------------------- G. the host API
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_predict_tokens_against_the_models_own_logits(packed):
    g = load_golden("small_h128_multitask")
    _, pcfg, sd = golden_cfg(g)
    B, S = g["labels"].shape
    nph, ntok = int(g["num_phonemes"]), int(g["num_tokens"])
    m = plbert_amd.MultiTaskModel(plbert_amd.AlbertModel(pcfg, max_batch=B, max_seq=S), nph, ntok, pcfg.hidden_size)
    inf = HipEngine(pcfg, nph, ntok, max_batch=B, max_seq=S, train=False)      # predict_tokens needs nothing a training engine has
    inf.load_state_dict(sd)
    m._engine = inf
    m.packed = packed
    m.eval()
    ids = torch.from_numpy(g["masked"])
    lens = g["lengths"].astype(np.int64)
    am = (~plbert_amd.length_to_mask(torch.Tensor(lens.tolist()))).int()
    with torch.no_grad():
        z_fwd = m(ids, attention_mask=am)[1].double().cpu().numpy()
        hid, _, _ = inf.forward(ids, inf._dev_i32(lens), want_hidden=True, want_phoneme=False)
    W = inf.view("token_predictor.weight").to(torch.bfloat16).double().cpu().numpy()
    bias = inf.view("token_predictor.bias").double().cpu().numpy()
    valid = (np.arange(S)[None, :] < lens[:, None])
    bound = (pcfg.hidden_size + 3) * 2.0 ** -23 * (np.abs(hid.double().cpu().numpy()) @ np.abs(W).T + np.abs(bias))
    for k in (5, 8):
        with torch.no_grad():
            got_ids, probs = m.predict_tokens(ids, attention_mask=am, topk=k)
        assert inf.grads is None and got_ids.dtype == torch.int64 and tuple(got_ids.shape) == (int(lens.sum()), k) == tuple(probs.shape)
        got, p = got_ids.cpu().numpy(), probs.cpu().numpy().astype(np.float64)
        zf, bd = z_fwd[valid], bound[valid].max(1)
        order = np.argsort(-zf, axis=1, kind="stable")
        top = np.take_along_axis(zf, order[:, :k + 1], 1)
        decided = (top[:, :-1] - top[:, 1:] > 2 * bd[:, None]).all(1)
        assert decided.mean() >= 0.9, decided.mean()
        assert np.array_equal(got[decided], order[decided, :k])
        picked = np.take_along_axis(zf, got, 1)
        assert bool((picked >= top[:, :k] - 2 * bd[:, None]).all())
        assert bool((p.sum(1) <= 1 + 1e-5).all()) and bool((np.diff(p, axis=1) <= 0).all())
        want_p = np.exp(picked - np.log(np.exp(zf - zf.max(1, keepdims=True)).sum(1, keepdims=True)) - zf.max(1, keepdims=True))
        assert bool((np.abs(p - want_p) <= 1e-4 * want_p + 1e-7).all())
    # explicit lists agree with positions=None; any order, a sample without positions
    positions = [[8, 1, 20], [], [2, 0]]
    with torch.no_grad():
        e_ids, e_p = m.predict_tokens(ids, attention_mask=am, positions=positions, topk=5)
        a_ids, a_p = m.predict_tokens(ids, attention_mask=am, topk=5)
    start = np.concatenate([[0], np.cumsum(lens)])
    pick = [int(start[b]) + i for b, ix in enumerate(positions) for i in ix]
    assert torch.equal(e_ids, a_ids[pick]) and torch.equal(e_p, a_p[pick])
    n_ids, n_p = m.predict_tokens(ids, attention_mask=am, positions=[[], [], []])
    assert tuple(n_ids.shape) == (0, 5) and tuple(n_p.shape) == (0, 5)
    with pytest.raises(ValueError, match="position outside"):
        m.predict_tokens(ids, attention_mask=am, positions=[[0], [33], [0]])


def test_validate_metrics_adds_the_token_keys_for_dual_head_batches_only(monkeypatch):
    from plbert_amd import run
    monkeypatch.setattr(run, "_batches", lambda loader, *a, **k: iter(loader))
    tr = _trainer()
    dual = [_dual_batch(tr, seed=s) for s in (41, 42)]
    m = run.validate_metrics(tr, dual)
    assert list(m) == ["val_phoneme_loss", "val_phoneme_acc", "val_phoneme_top5", "val_token_acc", "val_token_top5"]
    exact = [tr.evaluate(b)["token_exact"].cpu().numpy() for b in dual]
    tot = np.sum(exact, axis=0)
    assert m["val_token_acc"] == tot[1] / tot[0] and m["val_token_top5"] == tot[2] / tot[0] and tot[0] == 2 * 88
    assert 0.0 <= m["val_token_acc"] <= m["val_token_top5"] <= 1.0
    # phoneme-only batches: today's dict exactly
    for b in dual:
        b.token_ids = None
    m0 = run.validate_metrics(tr, dual)
    assert list(m0) == ["val_phoneme_loss", "val_phoneme_acc", "val_phoneme_top5"]
    assert list(run.validate_metrics(tr, dual, topk=3)) == ["val_phoneme_loss", "val_phoneme_acc", "val_phoneme_top3"]
