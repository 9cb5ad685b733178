"""Call-history independence (-m gpu): every engine call equals the same call on a freshly created engine, bit for bit.

Workspace buffers are carved per call and reused across calls; a call on T tokens runs most launches over Tp = ceil128(T)
rows (128-row slots per sample when token-packed), and the weight-gradient GEMMs, the column-sum partials and the 1-byte
images read every one of those rows. Rows T..Tp, the end of a packed slot, key rows at or past S inside a slot and the
columns NT..NTp of the token head belong to no token: DESIGN.md, "Rows and columns no token owns", lists who keeps each
of them harmless and which case below fails when that line is removed. A gradient row that is exactly zero times a finite
stale activation adds exactly zero to an fp32 sum, so nothing here has a tolerance: loss, outputs and gradient buffer are
compared as bit patterns (gpu_util.first_difference names the tensor and the coordinate of a difference).

One helper drives every case: a HISTORY runs on one engine, its gradient buffer is filled with 7.0 (a probe that
accumulated instead of overwriting would show), then the PROBE runs there and on a fresh engine built from the same
deterministic_state_dict. A fresh engine's result is a pure function of the probe, so it is computed once per probe and
shared, never modified.

Config A (bf16): vocab 188, embedding 128, hidden 256, 4 heads, FFN 512, 3 applications, token head of 1,000 classes
(NTp = 1,024: 24 padding columns), capacity 8 x 256. H = 256 reaches the fused GEMM + LayerNorm forms when Tp % 1024 == 0
and the gelu-derivative stash when Tp % 256 == 0. Config B (fp8): hidden 768, 12 heads, FFN 2048, 2 applications, 4 x 256.

About P5. B = 5, S = 90 cannot run token-packed: five 128-row slots are 640 rows, the padded call has 512, and a plan that
saves nothing IS the padded layout (plb_packing_plan). P5 is kept as specified — a call that is GIVEN a plan — and its
case asserts that it ran padded. P5w carries what P5 was meant for: the same lengths in S = 250, which does pack (five
slots = 640 rows, rounded to 1,024 of the padded call's 1,280: a 384-row tail), every slot one 128-row tile,
S % 128 != 0. The class of fault that commit e435a68 fixed (no dK / dV row stored at or past position S inside the slot of
a full-length sample) needs a full-length sample with S % 128 != 0: that is P6."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_util import assert_same_bits
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import HipEngine, packing_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NT = 1000
CFG_A = dict(vocab_size=188, embedding_size=128, hidden_size=256, num_attention_heads=4, intermediate_size=512,
             num_hidden_layers=3)
CAP_A = (8, 256)
CFG_B = dict(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048, num_hidden_layers=2,
             max_position_embeddings=512)
CAP_B = (4, 256)
P1_LENS = [90, 77, 64, 13, 1]
_SD = {}


def _engine(which="A"):
    cfg = plbert_amd.AlbertConfig(**(CFG_A if which == "A" else CFG_B))
    nt = NT if which == "A" else 0
    if which not in _SD:
        _SD[which] = plbert_amd.deterministic_state_dict(cfg, 188, nt, seed=5)
    B, S = CAP_A if which == "A" else CAP_B
    eng = HipEngine(cfg, 188, nt, max_batch=B, max_seq=S)
    eng.load_state_dict(_SD[which])
    return eng


# ---- batches -------------------------------------------------------------------------------------------------------------
def _ragged(B, S, lengths, seed, empty=(), share=7):
    """Ragged batch: ids 1..184 on the valid positions, zeros behind them; 1/share of every sample's positions masked
    (samples in ``empty``: none)."""
    rs = np.random.RandomState(seed)
    labels, masked, idx = np.zeros((B, S), np.int64), np.zeros((B, S), np.int64), []
    for b, n in enumerate(lengths):
        labels[b, :n] = rs.randint(1, 185, size=n)
        masked[b, :n] = labels[b, :n]
        ii = sorted(rs.choice(n, size=max(1, n // share), replace=False).tolist()) if b not in empty else []
        masked[b, ii] = 185
        idx.append(ii)
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    return SimpleNamespace(B=B, S=S, masked=masked, labels=labels, lens=np.asarray(lengths, np.int32), off=off, flat=flat,
                           n=int(off[-1]), tok=np.random.RandomState(seed + 1).randint(0, NT, size=(B, S)))


def _full(B, S, seed):
    """Full capacity, every position valid, two thirds of the positions masked: every activation row and every gradient row
    of every application holds real, non-zero values afterwards (more than half masked: nothing is pruned)."""
    labels, masked, _, idx = plbert_amd.synthetic_batch(B, S, seed=seed, word_pred_prob=0.9)
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    return SimpleNamespace(B=B, S=S, masked=masked, labels=labels, lens=None, off=off, flat=flat, n=int(off[-1]),
                           tok=np.random.RandomState(seed + 1).randint(0, NT, size=(B, S)))


def _loss_args(bt):
    return (bt.masked, bt.labels, bt.lens, bt.off, bt.flat, bt.n)


def _plan(bt, packs):
    plan = packing_plan(bt.lens, bt.S).to(DEV, non_blocking=False)
    assert plan.packed == packs, (plan.rows, bt.B * bt.S)
    return plan


def _ran(eng, bt, plan=None):
    """The layout the call ran in is the one the case exists for."""
    rows, of = eng.last_call_rows()
    assert of == bt.B * bt.S and rows == (plan.rows if plan is not None and plan.packed else of), (rows, of)


def _d_hidden(bt, H, seed):
    d = torch.randn((bt.B, bt.S, H), generator=torch.Generator().manual_seed(seed)) * 1e-2
    if bt.lens is not None:   # pad positions of d_hidden are ignored: NaN there, the same bits on both engines
        d[torch.as_tensor(np.arange(bt.S)[None, :] >= bt.lens[:, None])] = float("nan")
    return d


def _fused_launches(eng, call):
    _lib.profile_enable(True)
    try:
        out = call()
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    return out, prof.get("gemm_nt_lnfwd", {}).get("launches", 0) + prof.get("gemm_nt_lnbwd", {}).get("launches", 0)


# ---- what a call leaves ------------------------------------------------------------------------------------------------
def _grads(eng, dual=False):
    out = {"grads": eng.grads[: eng.trainable].clone()}
    if dual:
        lo, hi = eng.token_range
        out["token_grads"] = eng.grads[lo:hi].clone()
    return out


def _train(eng, bt, plan=None, dual=False, pruned=None):
    loss = eng.loss_fwd_bwd(*_loss_args(bt), token_ids=bt.tok if dual else None, packing=plan).clone()
    _ran(eng, bt, None if dual else plan)
    if pruned is not None:
        rows, of = eng.last_application_rows()
        assert (rows < of) == pruned, (rows, of)
    out = {"loss": loss, **_grads(eng, dual)}
    if dual:
        out["loss_parts"] = eng.loss_parts.clone()
    return out


# ---- histories: each at full capacity --------------------------------------------------------------------------------------
def h1(eng):
    """One padded loss_fwd_bwd, 8 x 256: T = 2,048 — the fused LayerNorm forms, the derivative stash."""
    (_, fused) = _fused_launches(eng, lambda: _train(eng, _full(8, 256, 41), pruned=False))
    assert fused == 6 + 5, fused   # 3 applications: 2 forward + 2 backward per application, minus the last LayerNorm-2 backward


def h2(eng):
    """One padded dual-head call: dirties the token head's logit gradient [Tp][NTp], its column partials and o_tgrad."""
    _train(eng, _full(8, 256, 42), dual=True)


def h3(eng):
    """encode + encode_bwd at 8 x 256, then another encode: every application's stash is kept and alive when the probe
    starts."""
    bt = _full(8, 256, 43)
    hid = eng.encode(bt.masked)
    eng.encode_bwd(_d_hidden(bt, hid.shape[-1], 44))
    eng.encode(bt.masked)


def h4(eng):
    """One token-packed loss_fwd_bwd, ragged: slots of 256, 128 and 128 rows after one another (1,664 used of 1,792 rows:
    a 128-row tail), so slot ends hold stale rows at positions the padded layout never uses. A third of the positions
    masked."""
    bt = _ragged(8, 256, [256, 100, 256, 57, 256, 256, 3, 256], 45, share=3)
    plan = _plan(bt, True)
    assert (plan.used, plan.rows) == (1664, 1792)
    _train(eng, bt, plan=plan)


def h5(eng):
    """forward(want_hidden, want_token) — the forward-only slot rotation, token logits — then H1."""
    bt = _full(8, 256, 46)
    eng.forward(bt.masked, None, want_hidden=True, want_token=True)
    h1(eng)


# ---- probes ----------------------------------------------------------------------------------------------------------------
def _bt_p1():   # one sample (13 tokens) without a masked index
    return _ragged(5, 90, P1_LENS, 3, empty=(3,))


def _bt_p5w():
    return _ragged(5, 250, P1_LENS, 4, empty=(3,))


def _bt_p6():
    return _ragged(4, 200, [200, 130, 128, 5], 6)


def p1(eng):
    """T = 450, Tp = 512: 62 ownerless rows, the unfused LayerNorm kernels, the derivative stash on, the pruned last
    application."""
    return _train(eng, _bt_p1(), pruned=True)


def p2(eng):
    """P1 with the last application on all rows: the unpruned layer loop has another set of memsets."""
    L = _lib.lib()
    L.plb_set_prune_last(0)
    try:
        return _train(eng, _bt_p1(), pruned=False)
    finally:
        L.plb_set_prune_last(-1)


def p3(eng):
    """T = 300, Tp = 384, Tp % 256 != 0: the derivative stash is off, the `act 2` epilogue reads u."""
    return _train(eng, _ragged(3, 100, [100, 57, 2], 7), pruned=True)


def p4(eng):
    """T = 1,024: the fused LayerNorm forms with no pad rows but with pad positions."""
    bt = _ragged(4, 256, [256, 256, 256, 201], 8)
    out, fused = _fused_launches(eng, lambda: _train(eng, bt, pruned=True))
    assert fused == 4 + 4, fused   # (the pruned last application's compact part runs on the small-shape launches)
    return out


def p4r(eng):
    """T = 1,000, Tp = 1,024: the fused LayerNorm forms WITH 24 ownerless rows (they have no Tzero: zero rows of the output
    gradient must come out as zero rows of dx and of the partials whatever mean / rstd / pre hold there)."""
    bt = _ragged(4, 250, [250, 250, 199, 250], 9)
    out, fused = _fused_launches(eng, lambda: _train(eng, bt, pruned=True))
    assert fused == 4 + 4, fused
    return out


def p5(eng):
    """S = 90 with a plan. It cannot pack (module docstring): runs padded, must equal a fresh engine's all the same."""
    bt = _bt_p1()
    return _train(eng, bt, plan=_plan(bt, False), pruned=True)


def p5w(eng):
    """Packed, the lengths of P1 in S = 250: every slot is one 128-row tile, S % 128 != 0; 640 used rows of 1,024 — a tail of
    384 rows, and a row count that takes the fused LayerNorm forms."""
    bt = _bt_p5w()
    plan = _plan(bt, True)
    assert (plan.used, plan.rows) == (640, 1024)
    return _train(eng, bt, plan=plan, pruned=True)


def p6(eng):
    """Packed, S = 200: a two-tile slot with a partial second tile whose rows 200..255 no backward kernel stores (the class
    of e435a68), a two-tile slot with two rows in the second tile, an exactly full tile, a nearly empty slot."""
    bt = _bt_p6()
    plan = _plan(bt, True)
    assert (plan.used, plan.rows) == (768, 768)
    return _train(eng, bt, plan=plan)


def p7(eng):
    """Dual-head padded call: columns NT..NTp, rows T..Tp of the fused cross-entropy passes, positions past the length."""
    return _train(eng, _ragged(3, 100, [100, 57, 2], 10), dual=True)


def _forward(eng, bt, plan, token):
    hid, ph, tk = eng.forward(bt.masked, bt.lens, want_hidden=True, want_token=token, packing=plan)
    _ran(eng, bt, None if token else plan)
    out = {"hidden": hid, "phoneme_logits": ph}
    if token:
        out["token_logits"] = tk
    return out


def p8_forward(eng):
    """forward with all three outputs at P1's shape, compared whole, pad positions included."""
    return _forward(eng, _bt_p1(), None, True)


def p8_forward_plan(eng):
    """The same call given a plan (token logits: runs padded)."""
    bt = _bt_p1()
    return _forward(eng, bt, _plan(bt, False), True)


def p8_forward_packed(eng):
    """Packed forward at P5w's shape: hidden and phoneme logits through the unpack kernels."""
    bt = _bt_p5w()
    return _forward(eng, bt, _plan(bt, True), False)


def _loss_only(eng, bt, plan, dual=False):
    eng._loss.fill_(-3.0)
    loss = eng.loss_fwd(*_loss_args(bt), token_ids=bt.tok if dual else None, packing=plan).clone()
    _ran(eng, bt, None if dual else plan)
    return {"loss": loss}


def p8_loss(eng):
    return _loss_only(eng, _bt_p1(), None)


def p8_loss_plan(eng):
    bt = _bt_p1()
    return _loss_only(eng, bt, _plan(bt, False))


def p8_loss_packed(eng):
    bt = _bt_p5w()
    return _loss_only(eng, bt, _plan(bt, True))


def p8_loss_dual(eng):
    """Loss-only dual-head call: pass 1 of the fused cross-entropy alone, one set of activation slots."""
    return _loss_only(eng, _ragged(3, 100, [100, 57, 2], 10), None, dual=True)


def _encode_pair(eng, bt, plan):
    hid = eng.encode(bt.masked, bt.lens, packing=plan)
    _ran(eng, bt, plan)
    eng.encode_bwd(_d_hidden(bt, hid.shape[-1], 11))
    torch.cuda.synchronize()
    out = {"hidden": hid, **_grads(eng)}
    assert bool(torch.isfinite(out["grads"]).all()), "a NaN of d_hidden's pad positions reached the gradients"
    return out


def p9(eng):
    """encode + encode_bwd at P1's shape, d_hidden NaN at the pad positions."""
    return _encode_pair(eng, _bt_p1(), None)


def p9_plan(eng):
    bt = _bt_p1()
    return _encode_pair(eng, bt, _plan(bt, False))


def p9_packed(eng):
    """... and token-packed at P5w's shape."""
    bt = _bt_p5w()
    return _encode_pair(eng, bt, _plan(bt, True))


def p9_packed_s200(eng):
    """... and at P6's shape: the unpruned packed backward with slot rows at or past S."""
    bt = _bt_p6()
    return _encode_pair(eng, bt, _plan(bt, True))


# ---- the driver ------------------------------------------------------------------------------------------------------------
_FRESH = {}


def _fresh(probe):
    if probe not in _FRESH:   # once per probe, shared, never modified
        eng = _engine()
        _FRESH[probe] = probe(eng)
        assert eng.status()["ln_exchange_timeouts"] == 0
    return _FRESH[probe]


def _compare(eng, got, want, what):
    assert got.keys() == want.keys()
    for k, a in got.items():
        b = want[k]
        assert a.shape == b.shape and a.dtype == torch.float32
        like = eng if k == "grads" else SimpleNamespace(layout={k: (0, a.numel(), tuple(a.shape))})
        if k == "token_grads":
            lo = eng.token_range[0]
            like = SimpleNamespace(layout={n: (o - lo, sz, shp) for n, (o, sz, shp) in eng.layout.items() if o >= lo})
        assert_same_bits(like, a, b, f"{k} of {what}")


def _check(history, probe):
    want = _fresh(probe)
    used = _engine()
    history(used)
    torch.cuda.synchronize()
    used.grads.fill_(7.0)
    got = probe(used)
    _compare(used, got, want, f"{probe.__name__} after {history.__name__}")
    assert used.status()["ln_exchange_timeouts"] == 0


ALL_PROBES = [p1, p2, p3, p4, p4r, p5, p5w, p6, p7, p8_forward, p8_forward_plan, p8_forward_packed, p8_loss, p8_loss_plan,
              p8_loss_packed, p8_loss_dual, p9, p9_plan, p9_packed, p9_packed_s200]
PAIRS = ([(h1, p) for p in ALL_PROBES]
         + [(h, p) for h in (h2, h3, h4, h5) for p in (p1, p5, p5w, p7)]
         # packed after packed with other slot maps; a layout switch in both directions
         + [(p6, p5), (p5, p6), (p6, p5w), (p5w, p6), (p5, p1), (p1, p5), (p5w, p1), (p1, p5w)])


@pytest.mark.parametrize("history,probe", PAIRS, ids=[f"{p.__name__}-after-{h.__name__}" for h, p in PAIRS])
def test_call_equals_a_fresh_engines(history, probe):
    _check(history, probe)


def test_the_fresh_result_is_repeatable():
    """What the matrix rests on: two fresh engines agree bit for bit (so any difference above is the history's)."""
    for probe in (p1, p6, p7):
        eng = _engine()
        _compare(eng, probe(eng), _fresh(probe), f"{probe.__name__} on a second fresh engine")


# ---- P10: fp8 -------------------------------------------------------------------------------------------------------------
def test_p10_fp8_calls_after_a_bf16_history_equal_a_fresh_engines():
    """Config B. The history (one full 4 x 256 call, T = 1,024, nothing pruned) runs in bf16; set_fp8(True) resets the
    scales; then the probe three times: the calibration call and two fp8 calls. B = 3, S = 200, lengths 200 / 151 / 9:
    T = 600, Tp = 640. The delayed-scaling state is a function of the stored rows only (the kernel tests hold every amax
    site to the maximum over the stored rows), so loss and gradients agree after EACH call, and fp8_stats at the end."""
    hist = _full(4, 256, 51)
    bt = _ragged(3, 200, [200, 151, 9], 12)
    res = {}
    for name in ("fresh", "used"):
        eng = _engine("B")
        if name == "used":
            eng.loss_fwd_bwd(*_loss_args(hist))
            rows, of = eng.last_application_rows()
            assert rows == of
            torch.cuda.synchronize()
            eng.grads.fill_(7.0)
        eng.set_fp8(True)
        calls = []
        for i in range(3):
            loss = eng.loss_fwd_bwd(*_loss_args(bt)).clone()
            calls.append({"loss": loss, **_grads(eng)})
            assert eng.fp8_state() == (True, True)
        res[name] = (eng, calls, eng.fp8_stats())
        assert eng.status()["ln_exchange_timeouts"] == 0
    eng, used, stats = res["used"]
    for i, (got, want) in enumerate(zip(used, res["fresh"][1])):
        _compare(eng, got, want, f"fp8 call {i} (0: calibration) after a bf16 history")
    assert not torch.equal(used[1]["grads"], used[0]["grads"])   # (the fp8 path did run: it is not the bf16 result)
    assert stats == res["fresh"][2], (stats, res["fresh"][2])
