"""-m gpu: which C entry point each public call reaches (plb_forward* / plb_encode* / plb_loss_*).

HipEngine and AlbertModel call the NARROWEST rung that carries what the caller gave: the error texts name the rung, and a
library named by PLBERT_HIP_LIB that predates a rung keeps serving the calls that do not need it. The test wraps ``engine.L``
in a recorder that logs the name of every such symbol it forwards, drives the public interface through every combination of
(per-application outputs, embedding inputs, key mask, and for the backward d_below / want_d_inputs_embeds), through the eight
(backward, dual, plan) loss calls and through AlbertModel.forward, and holds the log to literal lists. Public interface and
``engine.L`` only: the literals were taken from the if-chains this table replaced and hold for any later selection code.

Tiny model (H 128, 2 heads, FFN 256, E 64, 2 applications), capacity 2 x 256, lengths (256, 60): a plan for these lengths
packs (384 rows against 512), so the ``_packed`` symbols are reached beside the plain ones.
"""
import itertools

import numpy as np
import pytest
import torch

import plbert_amd
from plbert_amd.engine import HipEngine, packing_plan

pytestmark = pytest.mark.gpu
B, S, H, E, NL = 2, 256, 128, 64, 2
LENGTHS = (256, 60)
SHAPE = dict(embedding_size=E, hidden_size=H, num_attention_heads=2, intermediate_size=256, num_hidden_layers=NL,
             max_position_embeddings=256, type_vocab_size=2)
PREFIXES = ("plb_forward", "plb_encode", "plb_loss_")


class Recorder:
    """``engine.L`` with a log of the encoder / loss entry points called through it."""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(PREFIXES):
            return fn

        def call(*args):
            self.log.append(name)
            return fn(*args)
        return call

    def take(self):
        out, self.log = self.log, []
        return out


def _cfg():
    return plbert_amd.AlbertConfig(vocab_size=188, **SHAPE)


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(_cfg(), 188, 300, max_batch=B, max_seq=S)
    e.load_state_dict(plbert_amd.deterministic_state_dict(_cfg(), 188, 300, seed=3))
    e.L = Recorder(e.L)
    return e


def _ids():
    ids = np.random.RandomState(5).randint(1, 186, size=(B, S)).astype(np.int64)
    for b, n in enumerate(LENGTHS):
        ids[b, n:] = 0
    return torch.from_numpy(ids)


def _hole_mask():
    m = np.zeros((B, S), np.int32)
    for b, n in enumerate(LENGTHS):
        m[b, :n] = 1
    m[0, 5] = m[1, 3] = 0   # holes below the extents: no prefix masks
    return torch.from_numpy(m)


def _plan(eng):
    p = packing_plan(LENGTHS, S)
    assert p.packed and p.rows == 384
    return p.to(eng.device)


def _given(inputs, mask):
    kw = {}
    if inputs:
        kw["token_type_ids"] = torch.zeros((B, S), dtype=torch.int64)
    if mask:
        kw["key_mask"] = _hole_mask()
    return kw


# (per-application outputs asked for, embedding inputs given, key mask given) -> the symbol
FORWARD_LAYERS = {
    (False, False, False): "plb_forward_layers", (True, False, False): "plb_forward_layers",
    (False, True, False): "plb_forward_inputs", (True, True, False): "plb_forward_inputs",
    (False, False, True): "plb_forward_masked", (True, False, True): "plb_forward_masked",
    (False, True, True): "plb_forward_masked", (True, True, True): "plb_forward_masked",
}
ENCODE = {
    (False, False, False): "plb_encode", (True, False, False): "plb_encode_layers",
    (False, True, False): "plb_encode_inputs", (True, True, False): "plb_encode_inputs",
    (False, False, True): "plb_encode_masked", (True, False, True): "plb_encode_masked",
    (False, True, True): "plb_encode_masked", (True, True, True): "plb_encode_masked",
}
# (embedding inputs of the live encode, its key mask, d_below given, want_d_inputs_embeds) -> the symbol
ENCODE_BWD = {
    (False, False, False, False): "plb_encode_bwd", (False, False, True, False): "plb_encode_bwd_layers",
    (False, False, False, True): "plb_encode_bwd_inputs", (False, False, True, True): "plb_encode_bwd_inputs",
    (True, False, False, False): "plb_encode_bwd_inputs", (True, False, True, False): "plb_encode_bwd_inputs",
    (True, False, False, True): "plb_encode_bwd_inputs", (True, False, True, True): "plb_encode_bwd_inputs",
    (False, True, False, False): "plb_encode_bwd_masked", (False, True, True, False): "plb_encode_bwd_masked",
    (False, True, False, True): "plb_encode_bwd_masked", (False, True, True, True): "plb_encode_bwd_masked",
    (True, True, False, False): "plb_encode_bwd_masked", (True, True, True, False): "plb_encode_bwd_masked",
    (True, True, False, True): "plb_encode_bwd_masked", (True, True, True, True): "plb_encode_bwd_masked",
}
# (backward, dual-head, plan given) -> the symbol
LOSS = {
    (False, False, False): "plb_loss_fwd", (False, True, False): "plb_loss_fwd",
    (False, False, True): "plb_loss_fwd_packed", (False, True, True): "plb_loss_fwd_packed",
    (True, False, False): "plb_loss_fwd_bwd", (True, True, False): "plb_loss_fwd_bwd_dual",
    (True, False, True): "plb_loss_fwd_bwd_packed", (True, True, True): "plb_loss_fwd_bwd_dual_packed",
}


def test_forward(eng):
    lens = torch.tensor(LENGTHS, dtype=torch.int32)
    eng.forward(_ids(), lens, want_hidden=True)
    eng.forward(_ids(), lens, want_hidden=True, packing=_plan(eng))
    eng.forward(_ids(), lens, want_hidden=True, want_phoneme=False, token_type_ids=torch.zeros((B, S), dtype=torch.int64))
    assert eng.L.take() == ["plb_forward", "plb_forward_packed", "plb_forward_inputs"]


@pytest.mark.parametrize("packed", [False, True])
def test_forward_layers(eng, packed):
    lens = torch.tensor(LENGTHS, dtype=torch.int32)
    for key in itertools.product([False, True], repeat=3):
        layers, inputs, mask = key
        eng.forward_layers(_ids(), lens, _plan(eng) if packed else None, hidden_states=layers, attentions=False,
                           want_hidden=True, **_given(inputs, mask))
        assert eng.L.take() == [FORWARD_LAYERS[key]], key


@pytest.mark.parametrize("packed", [False, True])
def test_encode_and_backward(eng, packed):
    lens = torch.tensor(LENGTHS, dtype=torch.int32)
    d = torch.full((B, S, H), 1e-3, device=eng.device)
    for layers, inputs, mask, below, want in itertools.product([False, True], repeat=5):
        eng.encode(_ids(), lens, _plan(eng) if packed else None,
                   layers=dict(hidden_states=True, attentions=False) if layers else None, **_given(inputs, mask))
        die = eng.encode_bwd(d, d_below=[d] * NL if below else None, want_d_inputs_embeds=want)
        assert (die is not None) == want
        assert eng.L.take() == [ENCODE[layers, inputs, mask], ENCODE_BWD[inputs, mask, below, want]], \
            (layers, inputs, mask, below, want)


def test_loss_calls(eng):
    lens = torch.tensor(LENGTHS, dtype=torch.int32)
    off, flat = plbert_amd.masked_indices_to_csr([[1, 5, 9], [2, 3]])
    off, flat = torch.from_numpy(off), torch.from_numpy(flat)
    for key in itertools.product([False, True], repeat=3):
        backward, dual, packed = key
        call = eng.loss_fwd_bwd if backward else eng.loss_fwd
        call(_ids(), _ids(), lens, off, flat, 5, token_ids=_ids() if dual else None, packing=_plan(eng) if packed else None)
        assert eng.L.take() == [LOSS[key]], key


# AlbertModel.forward: (case, differentiable path) -> the symbols of the forward and, on that path, of the backward
MODEL = {
    ("plain", False): ["plb_forward"], ("plain", True): ["plb_encode", "plb_encode_bwd"],
    ("output_hidden_states", False): ["plb_forward_layers"],
    ("output_hidden_states", True): ["plb_encode_layers", "plb_encode_bwd_layers"],
    ("token_type_ids", False): ["plb_forward_inputs"], ("token_type_ids", True): ["plb_encode_inputs", "plb_encode_bwd_inputs"],
    ("inputs_embeds", False): ["plb_forward_inputs"], ("inputs_embeds", True): ["plb_encode_inputs", "plb_encode_bwd_inputs"],
    ("hole_mask", False): ["plb_forward_masked"], ("hole_mask", True): ["plb_encode_masked", "plb_encode_bwd_masked"],
}


@pytest.mark.parametrize("finetune", [False, True])
def test_albert_model(finetune):
    m = plbert_amd.AlbertModel(_cfg(), max_batch=B, max_seq=S, finetune=finetune)
    m.packed = False
    m.train(finetune)
    m.engine.L = rec = Recorder(m.engine.L)
    dev = m.engine.device
    prefix = torch.from_numpy((np.arange(S)[None, :] < np.asarray(LENGTHS)[:, None]).astype(np.int32))
    xe = torch.zeros((B, S, E), device=dev, requires_grad=True)
    cases = {
        "plain": dict(input_ids=_ids(), attention_mask=prefix),
        "output_hidden_states": dict(input_ids=_ids(), attention_mask=prefix, output_hidden_states=True),
        "token_type_ids": dict(input_ids=_ids(), attention_mask=prefix, token_type_ids=torch.zeros((B, S), dtype=torch.int64)),
        "inputs_embeds": dict(inputs_embeds=xe, attention_mask=prefix),
        "hole_mask": dict(input_ids=_ids(), attention_mask=_hole_mask()),
    }
    for name, kw in cases.items():
        out = m(**kw)
        if finetune:
            out.last_hidden_state.sum().backward()
            m.zero_grad(set_to_none=True)
        assert rec.take() == MODEL[name, finetune], name
    assert (xe.grad is not None) == finetune
    # a module with ``packed`` set follows a plan of the mask's lengths: the plain inference call is then the packed symbol
    if not finetune:
        m.packed = True
        m(input_ids=_ids(), attention_mask=prefix)
        assert rec.take() == ["plb_forward_packed"]
