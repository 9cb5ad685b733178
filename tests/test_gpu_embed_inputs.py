"""token_type_ids / position_ids / inputs_embeds through the C ABI (-m gpu): plb_forward_inputs, plb_encode_inputs and
plb_encode_bwd_inputs on the small model of tests/test_gpu_encode.py::_case_k with type_vocab_size = 3, against the float64
reference of tests/embed_inputs_ref.py (the oracle driven through a synthetic word table), against the plain calls, packed
against padded, and their refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import embed_inputs_ref as ref
import plbert_amd
from gpu_util import rel_l2, stream
from oracle import albert_np as onp
from plbert_amd import _lib
from plbert_amd.engine import HipEngine, packing_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY_BIAS = "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.key.bias"
QUERY_BIAS = KEY_BIAS.replace("key", "query")
K_SHAPE = (5, 300, [300, 129, 128, 65, 1])
NTY, NPOS, E, H = 3, 512, 64, 128
SETS = {"types": (True, False, False), "positions": (False, True, False), "embeds": (False, False, True),
        "all": (True, True, True)}


def _err():
    return _lib.lib().plb_last_error().decode()


def _case():
    B, S, lengths = K_SHAPE
    shape = dict(embedding_size=E, hidden_size=H, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2,
                 max_position_embeddings=NPOS, type_vocab_size=NTY)
    ocfg = onp.Config(**shape)
    pcfg = plbert_amd.AlbertConfig(vocab_size=188, **shape)
    sd = plbert_amd.deterministic_state_dict(pcfg, 188, seed=13)
    assert sd[ref.TYPE].shape == (NTY, E)
    rs = np.random.RandomState(100 * B + S)
    ids = np.zeros((B, S), np.int64)
    for b, n in enumerate(lengths):
        ids[b, :n] = rs.randint(1, 186, size=n)
    eng = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S)
    eng.load_state_dict(sd)
    return eng, ocfg, sd, ids, np.asarray(lengths, np.int32)


def _inputs(which, ids):
    B, S, lens = K_SHAPE
    tt, pid, xe = ref.inputs(B, S, lens, NTY, NPOS, E, 31)
    use_tt, use_pid, use_xe = SETS[which]
    return dict(ids=None if use_xe else ids, token_type_ids=tt if use_tt else None, position_ids=pid if use_pid else None,
                inputs_embeds=xe if use_xe else None)


def _plan(lens, S):
    plan = packing_plan(lens, S).to(DEV, non_blocking=False)
    assert plan.packed
    return plan


def _valid(lens, S):
    return np.arange(S)[None, :] < np.asarray(lens)[:, None]


def _dh(seed):
    B, S, lens = K_SHAPE
    d = np.random.RandomState(seed).randn(B, S, H) * 1e-2
    d[~_valid(lens, S)] = 0.0
    return d


_REF = {}


def _reference(which, ocfg, sd, ids, lens):
    if which not in _REF:   # computed once, shared, never modified
        kw = _inputs(which, ids)
        if kw["inputs_embeds"] is not None:
            kw["inputs_embeds"] = kw["inputs_embeds"].astype(np.float64)
        _REF[which] = ref.reference(ocfg, sd, lens, _dh(21), **kw)
    return _REF[which]


def _pair(eng, kw, lens, plan, dh, want_die=True):
    ids = kw["ids"]
    rest = {k: v for k, v in kw.items() if k != "ids"}
    hid = eng.encode(ids, lens, packing=plan, **rest)
    die = eng.encode_bwd(torch.as_tensor(dh, dtype=torch.float32), want_d_inputs_embeds=want_die)
    torch.cuda.synchronize()
    return hid, die


@pytest.mark.parametrize("which", sorted(SETS))
def test_hidden_and_gradients_against_the_reference(which):
    """The rules of test_gpu_encode.py::test_encode_bwd_gradients_against_the_oracle: per-tensor relative L2 4e-2; the key
    bias (true gradient 0): norm below 2e-2 of the query-bias gradient's. With inputs_embeds the word table's range is
    written as zeros: exactly. Every row of the token-type table is held to the bound on its own, not row 0 alone."""
    eng, ocfg, sd, ids, lens = _case()
    B, S = ids.shape
    want_h, G, want_die = _reference(which, ocfg, sd, ids, lens)
    kw = _inputs(which, ids)
    plan = _plan(lens, S)
    v = _valid(lens, S)
    hs, at, hid = eng.forward_layers(kw["ids"], lens, plan, hidden_states=False, want_hidden=True,
                                     **{k: x for k, x in kw.items() if k != "ids"})
    r = rel_l2(hid.cpu()[torch.as_tensor(v)], torch.as_tensor(want_h[v]))
    print(f"hidden (valid positions): rel L2 {r:.3e}")
    assert r < 4e-2
    eng.grads.fill_(7.0)                                      # overwritten, not accumulated
    d = _dh(21).copy()
    d[~v] = float("nan")                                      # pad positions of d_hidden are ignored
    hid2, die = _pair(eng, kw, lens, plan, d)
    assert torch.equal(hid2[torch.as_tensor(v).to(DEV)].view(torch.int32), hid[torch.as_tensor(v).to(DEV)].view(torch.int32))
    rows, of = eng.last_call_rows()
    assert rows < of and rows == plan.rows
    assert set(G) == {k for k in eng.layout if k.startswith("encoder.") and "pooler" not in k}
    worst = {}
    for k, want in G.items():
        got = eng.view(k, of=eng.grads).cpu()
        if k == KEY_BIAS:
            scale = float(eng.view(QUERY_BIAS, of=eng.grads).double().norm())
            assert float(got.double().norm()) < 2e-2 * scale, (k, float(got.double().norm()), scale)
            continue
        if k == ref.WORD and kw["inputs_embeds"] is not None:
            assert not want.any() and not bool(got.view(torch.int32).any())
            continue
        worst[k] = rel_l2(got, torch.as_tensor(want))
        print(f"{k}: rel L2 {worst[k]:.3e}")
    gt = eng.view(ref.TYPE, of=eng.grads).cpu()
    for row in range(NTY):
        if G[ref.TYPE][row].any():
            worst[f"{ref.TYPE}[{row}]"] = rel_l2(gt[row], torch.as_tensor(G[ref.TYPE][row]))
        else:
            assert not bool(gt[row].view(torch.int32).any())
    assert (G[ref.TYPE][1:].any()) == SETS[which][0]
    worst["d_inputs_embeds"] = rel_l2(die.cpu()[torch.as_tensor(v)], torch.as_tensor(want_die[v]))
    print({k: f"{x:.3e}" for k, x in worst.items() if "[" in k or k == "d_inputs_embeds"})
    bad = {k: x for k, x in worst.items() if not x < 4e-2}
    assert not bad, bad
    assert not bool(die.cpu()[torch.as_tensor(~v)].view(torch.int32).any())
    assert not bool(eng.view(ref.WORD, of=eng.grads)[0].view(torch.int32).any())
    head0 = eng.layout["phoneme_predictor.weight"][0]
    assert float(eng.grads[head0:eng.trainable].abs().max()) == 0.0 and eng.trainable > head0
    assert eng.status()["ln_exchange_timeouts"] == 0


def _check_sum(got, keys, terms, nrows, what):
    """got[row] against the float64 sum of the fp32 `terms` by key, element by element, within n * 2^-24 * sum|terms|."""
    want = torch.zeros(nrows, terms.shape[1], dtype=torch.float64).index_add_(0, keys, terms)
    mag = torch.zeros(nrows, terms.shape[1], dtype=torch.float64).index_add_(0, keys, terms.abs())
    n = torch.zeros(nrows, dtype=torch.float64).index_add_(0, keys, torch.ones(len(keys), dtype=torch.float64))
    err = (got.double() - want).abs()
    bound = n[:, None] * 2.0 ** -24 * mag
    print(f"{what}: largest error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_explicit_defaults_against_the_plain_call(layout):
    eng, ocfg, sd, ids, lens = _case()
    B, S = ids.shape
    plan = _plan(lens, S) if layout == "packed" else None
    dh = _dh(22)
    hid0 = eng.encode(ids, lens, packing=plan)
    eng.encode_bwd(torch.as_tensor(dh, dtype=torch.float32))
    torch.cuda.synchronize()
    g0 = eng.grads[: eng.trainable].clone()
    kw = dict(ids=ids, token_type_ids=np.zeros((B, S), np.int64), position_ids=np.tile(np.arange(S), (B, 1)), inputs_embeds=None)
    hid1, die = _pair(eng, kw, lens, plan, dh)
    assert torch.equal(hid1.view(torch.int32), hid0.view(torch.int32))
    g1 = eng.grads[: eng.trainable]
    v = torch.as_tensor(_valid(lens, S))
    terms = die.cpu().double()[v]
    s_of = torch.arange(S).expand(B, S)[v]
    for k, (o, sz, shp) in eng.layout.items():
        if o + sz > eng.trainable:
            continue
        if k in (ref.POS, ref.TYPE):   # two fixed orders of one sum: each within the bound of the exact sum
            keys = s_of if k == ref.POS else torch.zeros(len(s_of), dtype=torch.int64)
            for g, who in ((g1, "explicit defaults"), (g0, "plain")):
                _check_sum(g[o:o + sz].view(shp).cpu(), keys, terms, shp[0], f"{k} ({who})")
        else:
            assert torch.equal(g1[o:o + sz].view(torch.int32), g0[o:o + sz].view(torch.int32)), k


def test_packed_against_padded_with_all_three_inputs():
    eng, ocfg, sd, ids, lens = _case()
    B, S = ids.shape
    kw = _inputs("all", ids)
    dh = _dh(23)
    v = torch.as_tensor(_valid(lens, S)).to(DEV)
    hid_pad, die_pad = _pair(eng, kw, lens, None, dh)
    assert eng.last_call_rows() == (B * S, B * S)
    g_pad = eng.grads[: eng.trainable].clone()
    plan = _plan(lens, S)
    hid_pk, die_pk = _pair(eng, kw, lens, plan, dh)
    assert eng.last_call_rows() == (plan.rows, B * S)
    g_pk = eng.grads[: eng.trainable]
    assert torch.equal(hid_pk[v].view(torch.int32), hid_pad[v].view(torch.int32))
    head0 = eng.layout["phoneme_predictor.weight"][0]
    for k, (o, sz, shp) in eng.layout.items():
        if o + sz > head0 or k == KEY_BIAS:
            continue
        if k == ref.WORD:
            assert not bool(g_pk[o:o + sz].view(torch.int32).any()) and not bool(g_pad[o:o + sz].view(torch.int32).any())
            continue
        r = rel_l2(g_pk[o:o + sz], g_pad[o:o + sz])
        print(f"{k}: packed vs padded rel L2 {r:.3e}")
        assert r < 1.5e-2, (k, r)
    r = rel_l2(die_pk[v], die_pad[v])
    print(f"d_inputs_embeds: packed vs padded rel L2 {r:.3e}")
    assert r < 1.5e-2
    assert not bool(die_pk[~v].view(torch.int32).any()) and not bool(die_pad[~v].view(torch.int32).any())


def test_a_plain_pair_after_an_inputs_pair_equals_a_fresh_engines():
    eng, ocfg, sd, ids, lens = _case()
    B, S = ids.shape
    plan = _plan(lens, S)
    dh = torch.as_tensor(_dh(24), dtype=torch.float32)
    _pair(eng, _inputs("all", ids), lens, plan, _dh(25))
    hid = eng.encode(ids, lens, packing=plan)
    eng.encode_bwd(dh)
    fresh = _case()[0]
    hid_f = fresh.encode(ids, lens, packing=plan)
    fresh.encode_bwd(dh)
    torch.cuda.synchronize()
    assert torch.equal(hid.view(torch.int32), hid_f.view(torch.int32))
    assert torch.equal(eng.grads[: eng.trainable].view(torch.int32), fresh.grads[: fresh.trainable].view(torch.int32))
    assert eng.last_call_rows() == fresh.last_call_rows()


@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_forward_inputs_with_layers_fills_the_last_slot_like_hidden(layout):
    eng, ocfg, sd, ids, lens = _case()
    B, S = ids.shape
    kw = _inputs("all", ids)
    hs, at, hid = eng.forward_layers(None, lens, _plan(lens, S) if layout == "packed" else None, hidden_states=True,
                                     attentions=True, want_hidden=True, **{k: x for k, x in kw.items() if k != "ids"})
    v = torch.as_tensor(_valid(lens, S)).to(DEV)
    nl = eng.cfg.num_hidden_layers
    assert len(hs) == nl + 1 and all(h is not None for h in hs) and len(at) == nl
    assert torch.equal(hs[nl][v].view(torch.int32), hid[v].view(torch.int32))
    assert not bool(hs[nl][~v].view(torch.int32).any()) and not torch.equal(hs[0][v], hs[nl][v])


def test_refusals_name_the_cause_and_leave_the_gradients_alone():
    eng, ocfg, sd, ids, lens = _case()
    B, S = ids.shape
    L, h = eng.L, eng.handle
    eng._ensure_synced()
    ids_d, lens_d = eng._dev_i64(ids), eng._dev_i32(lens)
    tt, pid, xe = (torch.as_tensor(x).to(DEV) for x in ref.inputs(B, S, lens, NTY, NPOS, E, 31))
    hid, d = torch.empty((B, S, H), device=DEV), torch.zeros((B, S, H), device=DEV)
    die = torch.empty((B, S, E), device=DEV)
    eng.grads.copy_(torch.randn(eng.total, device=DEV))
    before = eng.grads.clone()
    both = _lib.PlbEmbedInputs(tt.data_ptr(), None, xe.data_ptr())
    types = _lib.PlbEmbedInputs(tt.data_ptr(), pid.data_ptr(), None)
    none = _lib.PlbEmbedInputs(None, None, None)

    def refused(rc, who, *words):
        assert rc != 0
        msg = _err()
        assert msg.startswith(who) and all(w in msg for w in words), msg
        torch.cuda.synchronize()
        assert torch.equal(eng.grads.view(torch.int32), before.view(torch.int32)), msg

    def fwd(fn, ids_p, inp):
        return fn(h, ids_p, None if inp is None else C.byref(inp), lens_d.data_ptr(), B, S, None, hid.data_ptr(), None, stream())

    def bwd(ids_p, inp, die_p=None):
        return L.plb_encode_bwd_inputs(h, ids_p, None if inp is None else C.byref(inp), lens_d.data_ptr(), B, S, None,
                                       d.data_ptr(), None, die_p, stream())

    for fn, who in ((L.plb_forward_inputs, "plb_forward_inputs"), (L.plb_encode_inputs, "plb_encode_inputs")):
        refused(fwd(fn, ids_d.data_ptr(), both), who, "both ids and inputs_embeds")
        refused(fwd(fn, None, types), who, "neither ids nor inputs_embeds")
        refused(fwd(fn, None, none), who, "ids is null")            # nothing given: the namesake's own refusal
        refused(fwd(fn, None, None), who, "ids is null")
    refused(L.plb_encode_inputs(h, ids_d.data_ptr(), C.byref(types), lens_d.data_ptr(), B, S, None, None, None, stream()),
            "plb_encode_inputs", "hidden is null")
    refused(bwd(ids_d.data_ptr(), types), "plb_encode_bwd_inputs", "no live plb_encode stash")
    assert fwd(L.plb_encode_inputs, ids_d.data_ptr(), types) == 0, _err()
    refused(bwd(ids_d.data_ptr(), both), "plb_encode_bwd_inputs", "both ids and inputs_embeds")
    refused(bwd(None, types), "plb_encode_bwd_inputs", "neither ids nor inputs_embeds")
    refused(bwd(None, None, die.data_ptr()), "plb_encode_bwd_inputs", "neither ids nor inputs_embeds")
    refused(L.plb_encode_bwd_inputs(h, ids_d.data_ptr(), C.byref(types), lens_d.data_ptr(), B, S, None, None, None, None, stream()),
            "plb_encode_bwd_inputs", "nothing to differentiate")
    assert bwd(ids_d.data_ptr(), types, die.data_ptr()) == 0, _err()     # the stash survived the refused calls
    torch.cuda.synchronize()
    assert not torch.equal(eng.grads[: eng.trainable], before[: eng.trainable])


def test_the_inputs_are_refused_in_fp8_mode():
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  num_hidden_layers=1, max_position_embeddings=512)
    eng = HipEngine(cfg, 188, 0, max_batch=1, max_seq=128)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(cfg, 188, seed=3))
    ids = np.random.RandomState(0).randint(1, 180, size=(1, 128))
    tt = np.ones((1, 128), np.int64)
    eng.set_fp8(True)
    before = eng.grads.clone()
    with pytest.raises(RuntimeError, match="plb_forward_inputs: fp8 mode is on"):
        eng.forward_layers(ids, hidden_states=False, want_hidden=True, token_type_ids=tt)
    with pytest.raises(RuntimeError, match="fp8 mode is on"):
        eng.encode(ids, token_type_ids=tt)
    assert torch.equal(eng.grads, before)
    eng.forward_layers(ids, hidden_states=False, want_hidden=True)      # the plain call keeps working in fp8 mode
    eng.set_fp8(False)
    eng.forward_layers(ids, hidden_states=False, want_hidden=True, token_type_ids=tt)


def test_happens_before_audit_of_an_inputs_pair():
    eng, ocfg, sd, ids, lens = _case()
    plan = _plan(lens, ids.shape[1])
    eng._bind()
    eng.hb_audit(True)
    _pair(eng, _inputs("all", ids), lens, plan, _dh(26))
    rep = eng.hb_report()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep
    eng.hb_audit(False)
