"""LAMB through the C ABI and Python (-m gpu): PLBertTrainer(optimizer="lamb"), HipEngine.lamb_step / trust_ratios,
plbert_amd.train.Lamb and the checkpoint, on the tiny engine: embedding 64, hidden 128, 2 heads, FFN 128, 2 layers, batch
2 x 64 (lengths 64 / 37), 188 phonemes, 8 tokens. Reference: the float64 restatement of tests/lamb_ref.py, driven by the engine's
own gradients — LAMB only reads the gradient buffer, so after a step it still holds what the loss call left.
Bounds: those of tests/test_gpu_lamb_kernel.py — 1e-5 relative on trust, and per element
|p_gpu - p_f64| <= ulp(p) / 2 + lr trust |u| (1e-5 + 4 x 2^-24), accumulated over the steps of a chain."""
import numpy as np
import pytest
import torch
from torch import nn

import lamb_ref as R
import plbert_amd
from plbert_amd import _lib
from plbert_amd.train import AdamW, Lamb, PLBertTrainer

pytestmark = pytest.mark.gpu

NAMES = _lib.PLB_PARAM_NAMES
EXCLUDE = ("bias", "LayerNorm", "layer_norm")
POSITION = "encoder.embeddings.position_embeddings.weight"


def _cfg():
    return plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=128, num_hidden_layers=2, max_position_embeddings=512)


def _ragged2(seed, S=64):
    labels, masked, _, idx = plbert_amd.synthetic_batch(2, S, seed=seed)
    lens = [S, 37]
    out = []
    for b, n in enumerate(lens):
        out.append([i for i in idx[b] if i < n] or [n // 2])
        labels[b, n:] = 0
        masked[b, n:] = 0
    return labels, masked, np.asarray(lens, np.int32), out


def _trainer(num_tokens=0, seed=8, **kw):
    sd = plbert_amd.deterministic_state_dict(_cfg(), 188, num_tokens, seed=seed)
    kw.setdefault("optimizer", "lamb")
    return PLBertTrainer(_cfg(), 188, max_batch=2, max_seq=64, lr=1e-3, state_dict=sd, num_tokens=num_tokens, **kw)


def _batch(tr, seed=41, tokens=False):
    lab, msk, lens, idx = _ragged2(seed)
    tok = np.random.RandomState(5).randint(0, 8, size=lab.shape).astype(np.int64) if tokens else None
    return tr.stage_batch(lab, msk, lens, idx, token_ids=tok)


def _snap(eng):
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().numpy().copy() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq))


def _plan(tr):
    """The plan of the NEXT optimizer step of the trainer (host only)."""
    groups, group_of = tr.groups_for_step()
    return tr.engine.lamb_plan(tr.step_count + 1, groups, group_of)


def _check_step(eng, before, plan, grad_scale=1.0, coef=None, chain=None):
    """One finished step against one float64 step from the state before it. ``chain`` (a dict carried from step to step):
    the float64 chain from the first state and the accumulated bound."""
    torch.cuda.synchronize()
    g = eng.grads.detach().cpu().numpy()
    ref = R.lamb_ref(before[0], g, before[1], before[2], plan, grad_scale, coef)
    p = eng.params.detach().cpu().numpy().astype(np.float64)
    ratios = eng.trust_ratios()
    assert set(ratios) == {NAMES[t["tensor"]] for t in plan}
    for k, t in enumerate(plan):
        name = NAMES[t["tensor"]]
        sl = slice(t["begin"], t["end"])
        wn, un, trust = (float(x) for x in ratios[name])
        for got, want, what in ((wn, ref["wn"][k], "wn"), (un, ref["un"][k], "un"), (trust, ref["trust"][k], "trust")):
            assert abs(got - want) <= R.TRUST_RTOL * want, (name, what, got, want)
        bound = R.p_bound(ref["p"][sl], ref["u"][sl], t["lr"], ref["trust"][k])
        assert (np.abs(p[sl] - ref["p"][sl]) <= bound).all(), (name, float(np.max(np.abs(p[sl] - ref["p"][sl]) / bound)))
        if not t["adapt"]:
            assert trust == 1.0, name
    if chain is not None:
        if not chain:
            chain.update(p=before[0].astype(np.float64), m=before[1].astype(np.float64), v=before[2].astype(np.float64),
                         bound=np.zeros(len(p)))
        c = R.lamb_ref(chain["p"], g, chain["m"], chain["v"], plan, grad_scale, coef)
        for k, t in enumerate(plan):
            sl = slice(t["begin"], t["end"])
            chain["bound"][sl] += R.p_bound(c["p"][sl], c["u"][sl], t["lr"], c["trust"][k])
        chain.update(p=c["p"], m=c["m"], v=c["v"])
        live = chain["bound"] > 0
        assert (np.abs(p - chain["p"])[live] <= chain["bound"][live]).all(), float(np.max(np.abs(p - chain["p"])[live] / chain["bound"][live]))
        assert np.array_equal(p[~live], chain["p"][~live])
    return ref


# ---- 1. three trainer steps -------------------------------------------------------------------------------------------------
def test_three_trainer_steps_against_the_restatement():
    tr = _trainer()
    eng = tr.engine
    batch = _batch(tr)
    assert tr.optimizer_entry_points() == ("plb_lamb_step",)
    assert sorted((g["weight_decay"], g["adapt"]) for g in tr.param_groups) == [(0.01, False), (0.01, True)]
    chain, p0 = {}, None
    for step in (1, 2, 3):
        before, plan = _snap(eng), _plan(tr)
        p0 = before[0] if p0 is None else p0
        assert [t["step"] for t in plan] == [step] * len(plan) and len(plan) == len([n for n in eng.layout if "pooler" not in n])
        assert all(bool(t["adapt"]) == (not any(x in NAMES[t["tensor"]] for x in EXCLUDE)) for t in plan)
        tr.step(batch)
        _check_step(eng, before, plan, chain=chain)
    assert tr.step_count == 3 and eng.status()["ln_exchange_timeouts"] == 0
    after = _snap(eng)[0]
    a, b = eng.layout["encoder.pooler.weight"][0], eng.layout["encoder.pooler.bias"][0] + eng.layout["encoder.pooler.bias"][1]
    assert np.array_equal(after[a:b], p0[a:b]) and not np.array_equal(after[:a], p0[:a])
    # the compute copies follow: a forward equals the forward of an engine that loaded the stepped parameters
    ids = np.random.RandomState(3).randint(1, 180, size=(2, 64))
    lens = np.asarray([64, 37], np.int32)
    fresh = _trainer()
    fresh.engine.load_state_dict(eng.state_dict())
    for x, y in zip(eng.forward(ids, lens), fresh.engine.forward(ids, lens)):
        assert (x is None and y is None) or torch.equal(x, y)
    # the moments are AdamW's, bit for bit: the clipped-free grouped AdamW step from the same state and gradients
    other = _trainer(optimizer="adamw", no_decay=("no such name",))
    lam = _trainer()
    for t in (other, lam):
        t.loss_and_grads(_batch(t))
    other.engine.grads.copy_(lam.engine.grads)
    for t in (other, lam):
        t._optimizer_step(1.0)
    torch.cuda.synchronize()
    assert torch.equal(other.engine.exp_avg, lam.engine.exp_avg) and torch.equal(other.engine.exp_avg_sq, lam.engine.exp_avg_sq)
    assert not torch.equal(other.engine.params, lam.engine.params)


# ---- 2. the token head -------------------------------------------------------------------------------------------------------
def test_dual_head_step_gives_the_token_head_its_own_count():
    tr = _trainer(num_tokens=8)
    eng = tr.engine
    ta, tb = eng.token_range
    dual, plain = _batch(tr, tokens=True), _batch(tr, seed=43)
    tr.step_count = 4                                                   # the encoder is at step 5, the token head at its first
    tr.loss_and_grads(dual)
    before, plan = _snap(eng), _plan(tr)
    tok = [t for t in plan if t["begin"] >= ta]
    assert [NAMES[t["tensor"]] for t in tok] == ["token_predictor.weight", "token_predictor.bias"]
    assert [t["step"] for t in tok] == [1, 1] and {t["step"] for t in plan if t["begin"] < ta} == {5}
    tr._dual = True
    tr._optimizer_step(1.0)
    _check_step(eng, before, plan)
    assert eng.token_head_steps == 1 and tr.step_count == 5
    assert not np.array_equal(_snap(eng)[0][ta:tb], before[0][ta:tb])
    # a phoneme-only step leaves it alone: bytes, count, and its slots are holes
    mid = _snap(eng)
    plan = None
    tr.step(plain)
    torch.cuda.synchronize()
    after = _snap(eng)
    for x, y in zip(mid, after):
        assert np.array_equal(x[ta:tb], y[ta:tb])
    assert eng.token_head_steps == 1 and "token_predictor.weight" not in eng.trust_ratios()
    res = eng.lamb_buf[:4 * _lib.PLB_NPARAM].view(-1, 4).cpu().numpy()
    assert not res[NAMES.index("token_predictor.weight")].any() and not res[NAMES.index("token_predictor.bias")].any()
    assert res[NAMES.index("phoneme_predictor.weight"), 3] == 1.0 and not res[NAMES.index("encoder.pooler.weight")].any()
    before, plan = _snap(eng), None
    tr.loss_and_grads(dual)
    plan = _plan(tr)
    assert [t["step"] for t in plan if t["begin"] >= ta] == [2, 2]
    tr._dual = True
    tr._optimizer_step(1.0)
    _check_step(eng, before, plan)
    assert eng.token_head_steps == 2 and eng.status()["ln_exchange_timeouts"] == 0


# ---- 3. frozen and no_decay ---------------------------------------------------------------------------------------------------
def test_frozen_and_no_decay_compose():
    tr = _trainer(frozen=("position_embeddings",), no_decay=EXCLUDE)
    eng = tr.engine
    assert sorted((g["weight_decay"], g["adapt"]) for g in tr.param_groups) == [(0.0, False), (0.01, True)]
    off, size, _ = eng.layout[POSITION]
    eng.exp_avg[off:off + size].fill_(123.25)
    eng.exp_avg_sq[off:off + size].fill_(321.5)
    batch = _batch(tr)
    tr.loss_and_grads(batch)
    # sentinels in the frozen tensor's bf16 copy, once the loss call has read it: a store would change them
    wb = eng.workspace[:2 * eng.total].view(torch.int16)          # the flat bf16 copy (tests/test_gpu_adamw_groups.py: _bf16_copy)
    wb[off:off + size] = 0x7FC1
    before, plan = _snap(eng), _plan(tr)
    wb0 = wb.clone()
    assert POSITION not in {NAMES[t["tensor"]] for t in plan}
    assert all((t["weight_decay"] == 0.0) == any(x in NAMES[t["tensor"]] for x in EXCLUDE) for t in plan)
    tr._optimizer_step(1.0)
    _check_step(eng, before, plan)
    after = _snap(eng)
    sl = slice(off, off + size)
    for x, y in zip(before, after):
        assert np.array_equal(x[sl].view(np.uint32), y[sl].view(np.uint32))
    assert torch.equal(wb[sl], wb0[sl]) and not torch.equal(wb[:off], wb0[:off])
    res = eng.lamb_buf[:4 * _lib.PLB_NPARAM].view(-1, 4).cpu().numpy()
    assert not res[NAMES.index(POSITION)].any() and POSITION not in eng.trust_ratios() and POSITION not in tr.stepped
    assert res[NAMES.index("encoder.embeddings.word_embeddings.weight"), 3] == 1.0


# ---- 4. clipping ---------------------------------------------------------------------------------------------------------------
def test_max_grad_norm_composes():
    tr = _trainer(max_grad_norm=1e-3)
    eng = tr.engine
    assert tr.optimizer_entry_points() == ("plb_grad_norm_groups", "plb_lamb_step")
    before, plan = _snap(eng), _plan(tr)
    tr.step(_batch(tr))
    torch.cuda.synchronize()
    norm = tr.last_grad_norm.cpu().numpy()
    assert 0.0 < norm[1] < 0.5 and norm[2] == 0.0 and norm[3] == 0.0
    _check_step(eng, before, plan, coef=norm[1])
    unclipped = _trainer()
    unclipped.step(_batch(unclipped))
    torch.cuda.synchronize()
    assert not torch.equal(unclipped.engine.exp_avg, eng.exp_avg)            # the coefficient reached the moments
    # an accumulated window: the mean of two micro-steps, one update
    acc = _trainer(max_grad_norm=1e-3)
    before, plan = _snap(acc.engine), _plan(acc)
    acc.step_accumulated([_batch(acc), _batch(acc, seed=43)])
    torch.cuda.synchronize()
    assert acc.step_count == 1
    _check_step(acc.engine, before, plan, grad_scale=0.5, coef=acc.last_grad_norm.cpu().numpy()[1])


# ---- 5. the fine-tune path -------------------------------------------------------------------------------------------------------
def test_finetune_path_updates_the_encoder_range_only():
    cfg = _cfg()
    bert = plbert_amd.AlbertModel(cfg, max_batch=2, max_seq=64, finetune=True)
    sd = plbert_amd.deterministic_state_dict(cfg, 188, 0, seed=8)
    bert.engine.load_state_dict({k: v for k, v in sd.items() if k.startswith("encoder.")}, strict=False)
    eng = bert.engine
    torch.manual_seed(0)
    lin = nn.Linear(cfg.hidden_size, 16).cuda()
    ids = torch.as_tensor(np.random.RandomState(3).randint(1, 180, size=(2, 64))).cuda()
    lens = torch.tensor([64, 37], device="cuda")
    mask = (torch.arange(64, device="cuda")[None, :] < lens[:, None]).int()
    opt = Lamb(bert.parameters(), lr=1e-3, model=bert)
    assert isinstance(opt, AdamW) and len(opt.param_groups) == 1 and opt.param_groups[0]["adapt"] is None
    opt.zero_grad()
    out = bert(ids, attention_mask=mask).last_hidden_state
    (lin(out) ** 2 * mask[..., None]).mean().backward()
    before = _snap(eng)
    groups, group_of = opt._live_groups()
    plan = eng.lamb_plan(1, groups, group_of)
    head0 = eng.layout["phoneme_predictor.weight"][0] if "phoneme_predictor.weight" in eng.layout else eng.layout["encoder.pooler.weight"][0]
    assert plan and max(t["end"] for t in plan) == head0 and {t["adapt"] for t in plan} == {0, 1}
    opt.step()
    _check_step(eng, before, plan)
    after = _snap(eng)
    for x, y in zip(before, after):
        assert np.array_equal(x[head0:], y[head0:])                              # the head, the pooler: untouched
    assert not np.array_equal(before[0][:head0], after[0][:head0]) and opt.step_count == 1
    sd_opt = opt.state_dict()
    assert sd_opt["param_groups"][0]["adapt"] is None and len(sd_opt["state"]) == len(plan)
    assert all(float(st["step"]) == 1.0 for st in sd_opt["state"].values())


# ---- 6. the checkpoint --------------------------------------------------------------------------------------------------------
def test_checkpoint_resumes_bitwise_and_refuses_the_other_optimizer(tmp_path):
    from plbert_amd import run as RUN
    tr = _trainer(no_decay=EXCLUDE)
    batch = _batch(tr)
    tr.step(batch)
    tr.step(batch)
    path = RUN.save_checkpoint(tr, 2, str(tmp_path), 0)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["optimizer_kind"] == "lamb"
    assert sorted((g["weight_decay"], g["adapt"]) for g in ck["optimizer"]["param_groups"]) == [(0.0, False), (0.01, True)]
    again = _trainer(seed=9, no_decay=EXCLUDE)
    assert RUN.load_checkpoint(again, path) == 2 and again.step_count == 2 and again.stepped == tr.stepped
    tr.step(batch)
    again.step(_batch(again))
    torch.cuda.synchronize()
    for what in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(tr.engine, what), getattr(again.engine, what)), what
    assert torch.equal(tr.engine.lamb_buf[:4 * _lib.PLB_NPARAM], again.engine.lamb_buf[:4 * _lib.PLB_NPARAM])
    adamw = _trainer(optimizer="adamw", no_decay=EXCLUDE)
    p0 = adamw.engine.params.clone()
    with pytest.raises(ValueError, match="written under optimizer 'lamb'"):
        RUN.load_checkpoint(adamw, path)
    assert torch.equal(adamw.engine.params, p0) and adamw.step_count == 0          # refused before anything was loaded
    RUN.load_checkpoint(adamw, path, restore_groups=False)                       # as a pretrained model it loads
    assert adamw.step_count == 2
    # and an AdamW file does not resume under LAMB
    plain = _trainer(optimizer="adamw")
    plain.step(_batch(plain))
    old = RUN.save_checkpoint(plain, 1, str(tmp_path), 0)
    assert "optimizer_kind" not in torch.load(old, map_location="cpu", weights_only=False)
    with pytest.raises(ValueError, match="written under optimizer 'adamw'"):
        RUN.load_checkpoint(_trainer(), old)
