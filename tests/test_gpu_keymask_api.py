"""-m gpu: attention masks that are no prefix, through the public interface (plb_*_masked, HipEngine, AlbertModel.forward).

Tiny model (H 128, 2 heads, E 64, I 128, L 2), B 3 x S 192, one batch with the three kinds of mask: sample 0 a LEFT PAD of 70
positions, sample 1 HOLES (key 0, keys 31..33, 64, 70..99; extent 120), sample 2 a PREFIX of 100 (extents
192 / 120 / 100: a packing plan of 512 rows for the 576 positions). The reference is
oracle.albert_np (float64), which takes any [B,S] mask as an additive bias, as transformers does
(tests/test_keymask_host.py holds it to transformers.AlbertModel under such masks).

Bounds, each taken from the existing comparison of the same quantity:
  last_hidden_state against the oracle, per element below the extent: 6e-2 (test_gpu_model_api.py, the H = 128 golden run);
      the PREFIX sample of this batch meets it as well, so the three are compared like for like;
  gradients of encode_bwd against oracle.encoder_backward: per tensor rel L2 4e-2, the key bias (true gradient 0) below 2e-2
      of the query-bias gradient's norm (test_gpu_encode.py::_check_against_oracle's rule);
  two bf16 evaluations of one function (left pad + position_ids against right pad): rel L2 1.5e-2
      (test_gpu_encode.py::test_packed_encode_bwd_equals_padded).
The weights are drawn at scale 0.08 (not the fixtures' 0.02) so that the scores have a spread and a wrong mask shows:
test_the_masks_matter holds the oracle with the mask replaced by its extent to be off by more than twice the forward bound.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import keymask_ref as R
import plbert_amd
from gpu_util import rel_l2, stream
from oracle import albert_np as onp
from plbert_amd import _lib
from plbert_amd.engine import HipEngine, packing_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, S, H, E, NL, NH = 3, 192, 128, 64, 2, 2
SHAPE = dict(embedding_size=E, hidden_size=H, num_attention_heads=NH, intermediate_size=128, num_hidden_layers=NL,
             max_position_embeddings=256, type_vocab_size=2)
KEY_BIAS = "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.key.bias"
QUERY_BIAS = KEY_BIAS.replace("key", "query")
HIDDEN_BOUND, GRAD_BOUND, KEY_BIAS_BOUND, TWO_EVAL_BOUND = 6e-2, 4e-2, 2e-2, 1.5e-2
LEFT = 70


def _masks():
    m = np.ones((B, S), np.int32)
    m[0, :LEFT] = 0
    m[1, [0, 31, 32, 33, 64]] = 0
    m[1, 70:100] = 0
    m[1, 120:] = 0
    m[2, 100:] = 0
    return m


MASK = _masks()
EXT = R.extents(torch.as_tensor(MASK)).numpy().astype(np.int32)
BELOW = np.arange(S)[None, :] < EXT[:, None]
VALID = (MASK != 0) & BELOW


def _ids():
    rs = np.random.RandomState(77)
    ids = rs.randint(1, 186, size=(B, S)).astype(np.int64)
    ids[~BELOW] = 0
    return ids


def _weights():
    pcfg = plbert_amd.AlbertConfig(vocab_size=188, **SHAPE)
    return pcfg, plbert_amd.deterministic_state_dict(pcfg, 188, seed=17, scale=0.08)


def _engine():
    pcfg, sd = _weights()
    eng = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S)
    eng.load_state_dict(sd)
    return eng


def _model(finetune):
    pcfg, sd = _weights()
    m = plbert_amd.AlbertModel(pcfg, max_batch=B, max_seq=S, finetune=finetune)
    m.engine.load_state_dict({k: v for k, v in sd.items() if k.startswith("encoder.")}, strict=False)
    return m


def _dh(seed):
    d = np.random.RandomState(seed).randn(B, S, H) * 1e-2
    d[~BELOW] = 0.0          # a hole keeps its gradient: it is a position like any other
    return d


_ORACLE = {}


def _oracle():
    if not _ORACLE:   # computed once, shared, never modified
        _, sd = _weights()
        ocfg = onp.Config(**SHAPE)
        hid, caches = onp.encoder_forward(ocfg, sd, _ids(), MASK, np.float64)
        _ORACLE["hidden"] = hid
        _ORACLE["grads"] = onp.encoder_backward(ocfg, sd, caches, _dh(5).astype(np.float64), np.float64)
        prefix_only = (np.arange(S)[None, :] < EXT[:, None]).astype(np.int32)
        _ORACLE["hidden_extent_only"], _ = onp.encoder_forward(ocfg, sd, _ids(), prefix_only, np.float64, keep=False)
    return _ORACLE


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_the_masks_matter():
    """The reference itself: with the left pad and the holes read as valid keys the hidden state moves by more than twice the
    bound the device is held to, in both masked samples (and not at all in the prefix sample)."""
    o = _oracle()
    d = np.abs(o["hidden"] - o["hidden_extent_only"])
    for b in (0, 1):
        print(f"sample {b}: mask ignored -> max abs {d[b][BELOW[b]].max():.3e}")
        assert d[b][BELOW[b]].max() > 2 * HIDDEN_BOUND
    assert d[2][BELOW[2]].max() == 0.0


@pytest.mark.parametrize("finetune", [False, True])
def test_forward_against_the_oracle(finetune):
    want = _oracle()["hidden"]
    m = _model(finetune)
    m.train(finetune)
    ids, am = torch.as_tensor(_ids()).to(DEV), torch.as_tensor(MASK).to(DEV)
    out = m(ids, attention_mask=am)
    hid = out.last_hidden_state.detach().cpu().numpy()
    assert out.last_hidden_state.requires_grad == finetune
    for b, kind in enumerate(("left pad", "holes", "prefix")):
        err = np.abs(hid[b] - want[b])[BELOW[b]].max()
        print(f"finetune={finetune} {kind}: max abs {err:.3e}")
        assert err < HIDDEN_BOUND, (kind, err)
    assert np.isfinite(hid).all()
    if finetune:
        assert not hid[~BELOW].any()                          # pads are zeros on the encode path
    # pooler_output is the pooler of position 0, a pad (sample 0) or a hole (sample 1) or not, as in transformers
    po = m.engine.pooler(out.last_hidden_state.detach())
    assert torch.equal(_bits(out.pooler_output), _bits(po))
    assert m.engine.last_call_rows() == (B * S, B * S)


def test_encode_bwd_gradients_against_the_oracle():
    G = _oracle()["grads"]
    eng = _engine()
    eng.grads.fill_(7.0)
    d = _dh(5).copy()
    d[~BELOW] = float("nan")                                  # pad positions of d_hidden are ignored
    hid = eng.encode(_ids(), EXT, key_mask=MASK)
    eng.encode_bwd(torch.as_tensor(d, dtype=torch.float32))
    torch.cuda.synchronize()
    assert not hid.cpu().numpy()[~BELOW].any()
    assert set(G) == {k for k in eng.layout if k.startswith("encoder.") and "pooler" not in k}
    worst = {}
    for k, want in G.items():
        got = eng.view(k, of=eng.grads).cpu()
        assert bool(torch.isfinite(got).all()), k
        if k == KEY_BIAS:
            scale = float(eng.view(QUERY_BIAS, of=eng.grads).double().norm())
            assert float(got.double().norm()) < KEY_BIAS_BOUND * scale, (k, float(got.double().norm()), scale)
            continue
        worst[k] = rel_l2(got, torch.as_tensor(want))
    print({k.split("albert_layers.0.")[-1]: f"{v:.3e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v < GRAD_BOUND}
    assert not bad, bad


def test_backward_through_the_module_fills_every_encoder_grad():
    m = _model(True)
    m.train()
    ids, am = torch.as_tensor(_ids()).to(DEV), torch.as_tensor(MASK).to(DEV)
    w = torch.as_tensor(_dh(6), dtype=torch.float32).to(DEV)
    out = m(ids, attention_mask=am, output_hidden_states=True)
    assert len(out.hidden_states) == NL + 1 and out.hidden_states[-1] is out.last_hidden_state
    ((out.last_hidden_state * w).sum() + (out.hidden_states[1] * w).sum()).backward()
    for n, p in m.named_parameters():
        if n.startswith("pooler"):
            assert p.grad is None
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), n
    # the same through the engine: the module's backward is plb_encode_bwd_masked on the live record
    eng = _engine()
    hid, hs, at = eng.encode(_ids(), EXT, key_mask=MASK, layers=dict(hidden_states=True, attentions=False))
    eng.encode_bwd(w, d_below=[None, w])
    torch.cuda.synchronize()
    assert torch.equal(_bits(hid), _bits(out.last_hidden_state.detach()))
    got = m.embeddings.word_embeddings.weight.grad
    assert torch.equal(_bits(got), _bits(eng.view("encoder.embeddings.word_embeddings.weight", of=eng.grads)))


def test_left_pad_with_position_ids_equals_right_pad():
    """The same tokens left-padded (position_ids = s - pad) and right-padded are one function evaluated twice."""
    m = _model(False)
    n = S - LEFT
    rs = np.random.RandomState(78)
    toks = rs.randint(1, 186, size=(B, n)).astype(np.int64)
    right_ids, left_ids = np.zeros((B, S), np.int64), np.zeros((B, S), np.int64)
    right_ids[:, :n], left_ids[:, LEFT:] = toks, toks
    right_am, left_am = np.zeros((B, S), np.int32), np.zeros((B, S), np.int32)
    right_am[:, :n], left_am[:, LEFT:] = 1, 1
    pid = np.clip(np.arange(S) - LEFT, 0, None)[None, :].repeat(B, 0)
    dev = lambda a: torch.as_tensor(a).to(DEV)
    right = m(dev(right_ids), attention_mask=dev(right_am)).last_hidden_state
    left = m(dev(left_ids), attention_mask=dev(left_am), position_ids=dev(pid)).last_hidden_state
    r = rel_l2(left[:, LEFT:], right[:, :n])
    print(f"left pad vs right pad: rel L2 {r:.3e}")
    assert r < TWO_EVAL_BOUND
    assert float((left[:, LEFT:] - right[:, :n]).abs().max()) < HIDDEN_BOUND


@pytest.mark.parametrize("finetune", [False, True])
def test_output_attentions_have_zero_columns_at_masked_keys(finetune):
    m = _model(finetune)
    m.train(finetune)
    ids, am = torch.as_tensor(_ids()).to(DEV), torch.as_tensor(MASK).to(DEV)
    out = m(ids, attention_mask=am, output_attentions=True, output_hidden_states=True)
    assert len(out.attentions) == NL
    valid, below = torch.as_tensor(VALID).to(DEV), torch.as_tensor(BELOW).to(DEV)
    for a in out.attentions:
        assert tuple(a.shape) == (B, NH, S, S) and bool(torch.isfinite(a).all())
        assert not bool(a[~valid[:, None, None, :].expand_as(a)].any())        # hole and pad columns: exact zeros
        assert not bool(a[~below[:, None, :, None].expand_as(a)].any())        # rows at and past the extent
        rows = below[:, None, :].expand(B, NH, S)
        assert float((a.double().sum(-1)[rows] - 1).abs().max()) <= 3e-3       # holes' own rows among them
    for h in out.hidden_states:
        assert not bool(h.detach()[~below].any())


def test_packed_equals_padded_and_a_prefix_mask_runs_as_before():
    m = _model(False)
    eng = m.engine
    ids, am = torch.as_tensor(_ids()).to(DEV), torch.as_tensor(MASK).to(DEV)
    below = torch.as_tensor(BELOW).to(DEV)
    pad = m(ids, attention_mask=am).last_hidden_state
    assert eng.last_call_rows() == (B * S, B * S)
    m.packed = True
    pk = m(ids, attention_mask=am).last_hidden_state
    plan = packing_plan(EXT, S)                                # the plan follows the extents; holes stay in their slot
    assert eng.last_call_rows() == (plan.rows, B * S) and plan.rows < B * S
    assert torch.equal(_bits(pk[below]), _bits(pad[below]))
    assert not bool(pk[~below].any())
    m.packed = False
    # a prefix mask: the lengths-only path, its calls and its bits
    prefix = torch.as_tensor(BELOW.astype(np.int32)).to(DEV)
    seen = []
    real = eng.forward_layers
    eng.forward_layers = lambda *a, **k: (seen.append(k.get("key_mask")), real(*a, **k))[1]
    got = m(ids, attention_mask=prefix).last_hidden_state
    eng.forward_layers = real
    assert seen == [] or seen == [None]
    want, _, _ = eng.forward(ids, torch.as_tensor(EXT), want_hidden=True, want_phoneme=False)
    assert eng.last_call_rows() == (B * S, B * S)
    assert torch.equal(_bits(got), _bits(want))
    # ... and the masked entry with the prefix as its key mask does the same arithmetic
    hs, at, hid = eng.forward_layers(ids, EXT, hidden_states=False, want_hidden=True, key_mask=BELOW.astype(np.int32))
    assert torch.equal(_bits(hid), _bits(want))


def test_a_plain_pair_after_a_masked_pair_equals_a_fresh_engines():
    eng, fresh = _engine(), _engine()
    ids = _ids()
    lens = np.array([192, 100, 7], np.int32)
    dh = torch.as_tensor(_dh(8), dtype=torch.float32)
    eng.encode(ids, EXT, key_mask=MASK)
    eng.encode_bwd(torch.as_tensor(_dh(9), dtype=torch.float32))
    eng.forward_layers(ids, EXT, hidden_states=False, attentions=True, key_mask=MASK)
    out = []
    for e in (eng, fresh):
        hid = e.encode(ids, lens)
        e.encode_bwd(dh)
        _, _, fwd = e.forward_layers(ids, lens, hidden_states=False, want_hidden=True)
        torch.cuda.synchronize()
        out.append((hid, e.grads[: e.trainable].clone(), fwd, e.last_call_rows()))
    for a, b in zip(out[0][:3], out[1][:3]):
        assert torch.equal(_bits(a), _bits(b))
    assert out[0][3] == out[1][3]


def test_refusals():
    eng = _engine()
    L, h = eng.L, eng.handle
    eng._ensure_synced()
    ids_d, ext_d = eng._dev_i64(_ids()), eng._dev_i32(EXT)
    km = torch.as_tensor(MASK).to(DEV)
    d = torch.zeros((B, S, H), device=DEV)
    hid = torch.empty((B, S, H), device=DEV)
    err = lambda: L.plb_last_error().decode()
    before = eng.grads.clone()

    def bwd(mask_p):
        return L.plb_encode_bwd_masked(h, ids_d.data_ptr(), None, mask_p, ext_d.data_ptr(), B, S, None, d.data_ptr(), None, None,
                                       stream())

    # a _bwd_masked call without a live stash
    assert bwd(km.data_ptr()) != 0 and err().startswith("plb_encode_bwd_masked") and "no live plb_encode stash" in err()
    # the backward takes the mask of its forward again: with a plain forward, or without the mask, it is refused
    assert L.plb_encode_masked(h, ids_d.data_ptr(), None, None, ext_d.data_ptr(), B, S, None, hid.data_ptr(), None, stream()) == 0
    assert bwd(km.data_ptr()) != 0 and "ran without one" in err(), err()
    assert L.plb_encode_masked(h, ids_d.data_ptr(), None, km.data_ptr(), ext_d.data_ptr(), B, S, None, hid.data_ptr(), None,
                               stream()) == 0
    assert bwd(None) != 0 and err().startswith("plb_encode_bwd_inputs") and "ran with one" in err(), err()
    torch.cuda.synchronize()
    assert torch.equal(_bits(eng.grads), _bits(before))
    assert bwd(km.data_ptr()) == 0, err()                     # the stash survived the refused calls
    # through the engine: a call in between ends the life of the record
    eng.encode(_ids(), EXT, key_mask=MASK)
    eng.forward(_ids(), EXT, want_phoneme=False)
    with pytest.raises(RuntimeError, match="no live plb_encode stash"):
        eng.encode_bwd(d)
    with pytest.raises(RuntimeError, match="no live encode"):
        eng.encode_bwd(d)
    with pytest.raises(ValueError, match="key_mask must be"):
        eng.forward_layers(_ids(), EXT, key_mask=MASK[:, :-1])
    # a mask row without a valid token
    m = _model(False)
    bad = torch.as_tensor(MASK).clone()
    bad[1] = 0
    with pytest.raises(ValueError, match="no valid token"):
        m(torch.as_tensor(_ids()).to(DEV), attention_mask=bad.to(DEV))


def test_a_mask_is_refused_in_fp8_mode():
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  num_hidden_layers=1, max_position_embeddings=512)
    eng = HipEngine(cfg, 188, 0, max_batch=1, max_seq=128)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(cfg, 188, seed=3))
    ids = np.random.RandomState(0).randint(1, 180, size=(1, 128))
    km = np.ones((1, 128), np.int32)
    km[0, 5] = 0
    eng.set_fp8(True)
    with pytest.raises(RuntimeError, match="plb_forward_masked: fp8 mode is on"):
        eng.forward_layers(ids, hidden_states=False, want_hidden=True, key_mask=km)
    with pytest.raises(RuntimeError, match="fp8 mode is on"):
        eng.encode(ids, key_mask=km)
    eng.forward_layers(ids, hidden_states=False, want_hidden=True)      # the plain call keeps working in fp8 mode
    eng.set_fp8(False)
    eng.forward_layers(ids, hidden_states=False, want_hidden=True, key_mask=km)


def test_head_wrappers_still_take_prefix_masks_only():
    pcfg, _ = _weights()
    m = plbert_amd.PhonemeOnlyModel(plbert_amd.AlbertModel(pcfg, max_batch=B, max_seq=S), 188, H)
    ids, am = torch.as_tensor(_ids()).to(DEV), torch.as_tensor(MASK).to(DEV)
    with pytest.raises(ValueError, match="must mark a prefix"):
        m(ids, attention_mask=am)
    with pytest.raises(ValueError, match="must mark a prefix"):
        m.fill_mask(ids, [[1], [2], [3]], attention_mask=am)
    out = m.encoder(ids, attention_mask=am).last_hidden_state            # the encoder itself takes the mask
    assert bool(torch.isfinite(out).all())
