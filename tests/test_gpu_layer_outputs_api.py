"""-m gpu: ``AlbertModel(..., finetune=True)(ids, attention_mask, output_hidden_states=True, output_attentions=True)`` — the
transformers arguments, on the small_h128 fixture (B = 3, S = 40, lengths 40 / 33 / 7, L = 2): the tuples, the identity of
the last slot, a loss built from a learned softmax-weighted sum of all slots (the layer-mixing front end of a downstream
model) whose backward reaches the encoder through plb_encode_bwd_layers, and the flag-less call as it always was."""
import numpy as np
import pytest
import torch

import layer_outputs_ref as lref
from oracle import albert_np as onp
from test_gpu_encode import KEY_BIAS, QUERY_BIAS
from test_gpu_finetune_api import _bert, _fixture
from gpu_util import rel_l2
from conftest import golden_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_flags_return_the_tuples_and_no_grad_gives_the_same_values():
    g, pcfg, sd, ids, mask = _fixture()
    nl = pcfg.num_hidden_layers
    bert = _bert(pcfg, sd, ids, finetune=True)
    out = bert(ids, attention_mask=mask, output_hidden_states=True, output_attentions=True)
    assert isinstance(out.hidden_states, tuple) and len(out.hidden_states) == nl + 1
    assert isinstance(out.attentions, tuple) and len(out.attentions) == nl
    assert out.last_hidden_state is out.hidden_states[-1]
    assert out[0] is out.last_hidden_state and out[1] is out.pooler_output and out[2] is out.hidden_states and out[3] is out.attentions
    assert all(h.requires_grad and tuple(h.shape) == (3, 40, pcfg.hidden_size) for h in out.hidden_states)
    assert all(not a.requires_grad and tuple(a.shape) == (3, pcfg.num_attention_heads, 40, 40) for a in out.attentions)
    assert not out.pooler_output.requires_grad
    for h in out.hidden_states:
        assert float(h.detach()[mask == 0].abs().max()) == 0.0
    with torch.no_grad():
        ng = bert(ids, attention_mask=mask, output_hidden_states=True, output_attentions=True)
    bert.eval()
    ev = bert(ids, attention_mask=mask, output_hidden_states=True, output_attentions=True)
    for other in (ng, ev):
        assert other.last_hidden_state is other.hidden_states[-1] and not other.last_hidden_state.requires_grad
        for a, b in zip(out.hidden_states + out.attentions + (out.pooler_output,),
                        other.hidden_states + other.attentions + (other.pooler_output,)):
            assert torch.equal(_bits(a.detach()), _bits(b))
    # one flag alone; the flags as None (transformers' default)
    only = bert.train()(ids, attention_mask=mask, output_attentions=True, output_hidden_states=None)
    assert only.hidden_states is None and len(only.attentions) == nl and only.last_hidden_state.requires_grad
    assert torch.equal(_bits(only.last_hidden_state.detach()), _bits(out.last_hidden_state.detach()))
    only.last_hidden_state.sum().backward()                    # the backward of a call that asked for maps only


def test_without_the_flags_the_output_is_what_it_was():
    g, pcfg, sd, ids, mask = _fixture()
    for finetune in (False, True):
        bert = _bert(pcfg, sd, ids, finetune=finetune)
        out = bert(ids, attention_mask=mask)
        assert out.hidden_states is None and out.attentions is None and len(out.to_tuple()) == 2
        assert out[0] is out.last_hidden_state and out[1] is out.pooler_output
        lens = mask.sum(1).to(torch.int32)
        if finetune:
            want = bert.engine.encode(ids, lens)
        else:
            want, _, _ = bert.engine.forward(ids, lens, want_hidden=True, want_phoneme=False)
        assert torch.equal(_bits(out.last_hidden_state.detach()), _bits(want))
        assert torch.equal(_bits(out.pooler_output), _bits(bert.engine.pooler(want)))


def test_a_learned_mix_of_all_slots_backpropagates():
    """loss = < T, sum_l softmax(w)_l hidden_states[l] >: the encoder's .grad against the float64 oracle through the identity
    of tests/test_layer_outputs_host.py with G_l = softmax(w)_l T (bounds of test_gpu_encode._check_against_oracle: 4e-2
    per tensor, key bias below 2e-2 of the query bias' norm); the mixing weights' gradient, which torch computes from the
    hidden states this library returned, against the oracle's hidden states."""
    g, pcfg, sd, ids, mask = _fixture()
    ocfg = golden_cfg(g)[0]
    nl, H = pcfg.num_hidden_layers, pcfg.hidden_size
    bert = _bert(pcfg, sd, ids, finetune=True)
    lens = np.asarray(g["lengths"], np.int32)
    v = lref.valid_mask(lens, 40)
    T = np.random.RandomState(3).randn(3, 40, H) * 1e-2 * v[..., None]
    w = torch.nn.Parameter(torch.tensor([0.3, -0.2, 0.5][: nl + 1], device=DEV))
    out = bert(ids, attention_mask=mask, output_hidden_states=True)
    mix = sum(c * h for c, h in zip(torch.softmax(w, 0), out.hidden_states))
    loss = (mix * torch.as_tensor(T, dtype=torch.float32, device=DEV)).sum()
    loss.backward()
    coef = torch.softmax(w.detach().double().cpu(), 0).numpy()
    hid, caches = onp.encoder_forward(ocfg, sd, np.asarray(g["masked"]), onp.attention_mask_from_lengths(lens), np.float64)
    want = lref.layer_gradient_sum(ocfg, sd, caches, [c * T for c in coef])
    eng = bert.engine
    seen = 0
    for n, p in bert.named_parameters():
        if n.startswith("pooler."):
            assert p.grad is None
            continue
        k = "encoder." + n
        assert p.grad is not None
        if k == KEY_BIAS:
            qb = dict(bert.named_parameters())[QUERY_BIAS[len("encoder."):]].grad
            assert float(p.grad.double().norm()) < 2e-2 * float(qb.double().norm())
        else:
            r = rel_l2(p.grad.cpu(), torch.as_tensor(want[k]))
            print(f"{k}: rel L2 {r:.3e}")
            assert r < 4e-2, (k, r)
        seen += 1
    assert seen == 23
    # d loss / d w_l = sum_m (d softmax_m / d w_l) <T, h_m>, from the oracle's hidden states
    dots = np.array([float((T * h).sum()) for h in lref.hidden_states_of(hid, caches)])
    dw = coef * (dots - float((coef * dots).sum()))
    # Every slot is within rel-L2 1e-2 of the oracle's (tests/test_gpu_layer_outputs.py), so |<T, dh_m>| <= 1e-2 |T| |h_m|, and
    # d w_l = c_l (dot_l - sum_m c_m dot_m) with c a probability vector moves by at most twice the largest of those.
    bound = 2 * 1e-2 * float(np.linalg.norm(T)) * max(float(np.linalg.norm(h * v[..., None])) for h in lref.hidden_states_of(hid, caches))
    print("mixing weights' gradient", w.grad.cpu().numpy(), "oracle", dw, "bound", bound)
    assert np.abs(w.grad.cpu().numpy() - dw).max() < bound
    assert eng.poll_status()["ln_exchange_timeouts"] == 0


def test_a_slot_nothing_uses_goes_in_as_null():
    """Only hidden_states[1] feeds the loss: the other slots' gradients arrive as None and the result is that of the engine
    called with that one slot."""
    g, pcfg, sd, ids, mask = _fixture()
    bert = _bert(pcfg, sd, ids, finetune=True)
    T = torch.as_tensor(np.random.RandomState(4).randn(3, 40, pcfg.hidden_size) * 1e-2, dtype=torch.float32, device=DEV)
    out = bert(ids, attention_mask=mask, output_hidden_states=True)
    (out.hidden_states[1] * T).sum().backward()
    head0 = bert.engine.layout["phoneme_predictor.weight"][0]
    got = bert.engine.grads[:head0].clone()
    eng = bert.engine
    eng.encode(ids, mask.sum(1).to(torch.int32))
    eng.encode_bwd(None, d_below=[None, T])
    assert torch.equal(_bits(got), _bits(eng.grads[:head0]))
    assert float(got.abs().max()) > 0
