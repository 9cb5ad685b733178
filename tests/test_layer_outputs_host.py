"""CPU checks behind the per-application outputs (output_hidden_states / output_attentions with gradients): the float64
references of tests/layer_outputs_ref.py against the oracle, the gradient identity the -m gpu tests rely on against central
finite differences, the output object of AlbertModel.forward on a stub engine, and the new ABI against the header."""
import numpy as np
import pytest
import torch

import c_header
import layer_outputs_ref as lref
from oracle import albert_np as onp
import plbert_amd
from plbert_amd import _lib
from plbert_amd.model import AlbertModel, BaseModelOutputWithPooling

LAYER = onp.LAYER


def _tiny(L=3, H=128, seed=5):
    """L = 3, H = 128 (2 heads of 64), B = 3, S = 7, lengths 7 / 4 / 1; weights N(0, 0.3) so that the attention maps are not
    flat and every term of the gradient is well above float64 noise."""
    ocfg = onp.Config(vocab_size=23, embedding_size=16, hidden_size=H, num_attention_heads=2, intermediate_size=48,
                      num_hidden_layers=L, max_position_embeddings=16)
    pcfg = plbert_amd.AlbertConfig(vocab_size=23, embedding_size=16, hidden_size=H, num_attention_heads=2,
                                   intermediate_size=48, num_hidden_layers=L, max_position_embeddings=16)
    rs = np.random.RandomState(seed)
    sd = {}
    for k, shp in plbert_amd.param_shapes(pcfg, 4).items():
        if k.startswith("encoder.") and "pooler" not in k:
            w = rs.randn(*shp) * 0.3
            sd[k] = 1.0 + w if k.endswith("LayerNorm.weight") or k.endswith("layer_norm.weight") else w
    lens = np.asarray([7, 4, 1], np.int32)
    ids = np.zeros((3, 7), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = rs.randint(1, 23, size=n)
    return ocfg, sd, ids, lens


def test_probability_reference_reproduces_the_oracle():
    ocfg, sd, ids, lens = _tiny()
    B, S = ids.shape
    _, caches = onp.encoder_forward(ocfg, sd, ids, onp.attention_mask_from_lengths(lens), np.float64)
    v = lref.valid_mask(lens, S)
    assert len(caches["layers"]) == 3
    for c in caches["layers"]:
        got = lref.attn_probs_ref(c["q"], c["k"], lens, 64 ** -0.5)
        want = c["pr"]
        rows = np.broadcast_to(v[:, None, :, None], want.shape)
        assert np.abs(got - want)[rows].max() < 1e-14        # valid query rows: every column, the pad ones (0 in both) included
        assert not got[~rows].any()                          # pad query rows: zeros here, values in the oracle
        assert not got[np.broadcast_to(~v[:, None, None, :], got.shape)].any()
        assert np.abs(got.sum(-1)[np.broadcast_to(v[:, None, :], got.shape[:3])] - 1).max() < 1e-14
    # maps of different applications differ: the reference is not insensitive to which q / k it is given
    assert np.abs(caches["layers"][0]["pr"] - caches["layers"][1]["pr"]).max() > 1e-2


def test_add_row_grad_reference():
    B, S, H, lens = 2, 5, 8, [5, 2]
    g = torch.randn(B, S, H)
    g[1, 2:] = float("nan")                                   # pads: never read
    res = torch.randn(128, H).to(torch.bfloat16)
    pos, rows = lref.token_rows(lens, S)
    assert pos.tolist() == [0, 1, 2, 3, 4, 5, 6] and rows.tolist() == pos.tolist()
    out = lref.add_row_grad_ref(res, g, pos, rows)
    assert not bool(out.float().isnan().any())
    assert torch.equal(out[7:], res[7:]) and torch.equal(out[:5], (res[:5].float() + g[0]).to(torch.bfloat16))
    assert torch.equal(out[5:7], (res[5:7].float() + g[1, :2]).to(torch.bfloat16))
    pos, rows = lref.token_rows(lens, S, row_start=[0, 128])  # a packed plan: sample 1 starts a slot of its own
    assert rows.tolist() == [0, 1, 2, 3, 4, 128, 129] and pos.tolist() == [0, 1, 2, 3, 4, 5, 6]


def test_gradient_identity_against_finite_differences():
    """d/dP sum_l <G_l, hidden_states[l]> = sum_l encoder_backward(l applications, caches[:l], G_l), in float64, on a few
    entries of every tensor; once with every slot, once with one inner slot alone (what the -m gpu tests feed)."""
    ocfg, sd, ids, lens = _tiny()
    B, S = ids.shape
    H, L = ocfg.hidden_size, ocfg.num_hidden_layers
    am = onp.attention_mask_from_lengths(lens)
    v = lref.valid_mask(lens, S)
    rs = np.random.RandomState(11)
    Gall = [rs.randn(B, S, H) * v[..., None] for _ in range(L + 1)]

    def objective(P, Gs):
        hid, caches = onp.encoder_forward(ocfg, P, ids, am, np.float64)
        return sum(float((G * h).sum()) for G, h in zip(Gs, lref.hidden_states_of(hid, caches)) if G is not None)

    hid, caches = onp.encoder_forward(ocfg, sd, ids, am, np.float64)
    hs = lref.hidden_states_of(hid, caches)
    assert len(hs) == L + 1 and hs[-1] is hid
    for Gs in (Gall, [None, None, Gall[2], None]):
        grads = lref.layer_gradient_sum(ocfg, sd, caches, Gs)
        assert set(grads) == set(sd)
        worst = 0.0
        for k, g in grads.items():
            if k == LAYER + "attention.key.bias":   # softmax is invariant to it: the true gradient is 0, both ways
                assert np.abs(g).max() < 1e-10 * np.abs(grads[LAYER + "attention.query.bias"]).max()
                continue
            flat = np.flatnonzero(np.abs(g.reshape(-1)) > 1e-3 * np.abs(g).max())
            assert flat.size, k
            for i in rs.choice(flat, size=min(3, flat.size), replace=False):
                h = 1e-5
                P = {n: (a.copy() if n == k else a) for n, a in sd.items()}
                P[k].reshape(-1)[i] += h
                up = objective(P, Gs)
                P[k].reshape(-1)[i] -= 2 * h
                fd = (up - objective(P, Gs)) / (2 * h)
                err = abs(fd - g.reshape(-1)[i]) / (abs(fd) + 1e-12)
                worst = max(worst, err)
                assert err < 1e-5, (k, int(i), fd, float(g.reshape(-1)[i]))
        print(f"worst relative difference to central differences: {worst:.2e}")
    # the one-slot form is not the all-slot form: the inner slot's term is a proper part of the sum
    one = lref.layer_gradient_sum(ocfg, sd, caches, [None, None, Gall[2], None])
    k = LAYER + "ffn.weight"
    assert np.abs(one[k] - lref.layer_gradient_sum(ocfg, sd, caches, Gall)[k]).max() > 1e-3 * np.abs(one[k]).max()


# ---- the output object ------------------------------------------------------------------------------------------------
class _StubEngine:
    """What AlbertModel.forward asks of its engine on the non-differentiable path."""

    def __init__(self, L, H, NH):
        self.L, self.H, self.NH, self.calls = L, H, NH, []

    def forward_layers(self, ids, lengths=None, packing=None, hidden_states=True, attentions=False, want_hidden=False):
        B, S = ids.shape
        self.calls.append(("forward_layers", hidden_states, attentions))
        hs = [torch.full((B, S, self.H), float(l)) if hidden_states else None for l in range(self.L + 1)]
        at = [torch.full((B, self.NH, S, S), float(l)) if attentions else None for l in range(self.L)]
        return (hs, at, torch.full((B, S, self.H), -1.0)) if want_hidden else (hs, at)

    def forward(self, ids, lengths=None, want_hidden=False, want_phoneme=True, want_token=False, packing=None):
        B, S = ids.shape
        self.calls.append(("forward",))
        return torch.full((B, S, self.H), -1.0), None, None

    def pooler(self, hidden):
        return hidden[:, 0] * 0.5


def _stub_model(L=3, H=128, NH=2):
    m = AlbertModel.__new__(AlbertModel)
    torch.nn.Module.__init__(m)
    m.config = plbert_amd.AlbertConfig(vocab_size=23, embedding_size=16, hidden_size=H, num_attention_heads=NH,
                                       intermediate_size=48, num_hidden_layers=L, max_position_embeddings=16)
    m._engine = _StubEngine(L, H, NH)
    m.differentiable = False
    return m.eval()


def test_output_object_follows_transformers():
    m = _stub_model()
    ids = torch.ones((2, 5), dtype=torch.int64)
    plain = m(ids)
    assert m._engine.calls == [("forward",)]                    # without the flags: the call it always made
    assert plain.hidden_states is None and plain.attentions is None and len(plain.to_tuple()) == 2
    assert plain[0] is plain.last_hidden_state and plain[1] is plain.pooler_output
    both = m(ids, output_hidden_states=True, output_attentions=True)
    assert m._engine.calls[-1] == ("forward_layers", True, True)
    assert isinstance(both.hidden_states, tuple) and len(both.hidden_states) == 4
    assert isinstance(both.attentions, tuple) and len(both.attentions) == 3
    assert both.last_hidden_state is both.hidden_states[-1]
    assert both[0] is both.last_hidden_state and both[1] is both.pooler_output
    assert both[2] is both.hidden_states and both[3] is both.attentions
    assert [float(h[0, 0, 0]) for h in both.hidden_states] == [0.0, 1.0, 2.0, 3.0]
    only_att = m(ids, output_attentions=True)
    assert only_att.hidden_states is None and only_att[2] is only_att.attentions      # None entries are skipped
    assert float(only_att.last_hidden_state[0, 0, 0]) == -1.0                         # the call's own `hidden`
    only_hs = m(ids, output_hidden_states=True, output_attentions=None)
    assert only_hs.attentions is None and len(only_hs.to_tuple()) == 3
    with pytest.raises(IndexError):
        only_hs[3]
    # the flags are arguments of their own now, not swallowed
    import inspect
    par = inspect.signature(AlbertModel.forward).parameters
    assert par["output_hidden_states"].default is False and par["output_attentions"].default is False
    o = BaseModelOutputWithPooling(last_hidden_state=torch.zeros(1))
    assert o.to_tuple() == (o.last_hidden_state,)


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_new_entry_points_match_the_header():
    hdr, khdr = c_header.public(), c_header.kernels()
    L = _lib.lib()
    for name in ("plb_forward_layers", "plb_encode_layers", "plb_encode_bwd_layers"):
        assert c_header.bound_mismatch(hdr, getattr(L, name), _lib) is None
    for name in ("plb_launch_attn_probs", "plb_launch_add_row_grad"):
        assert c_header.bound_mismatch(khdr, getattr(L, name), _lib) is None
    assert [f.name for f in hdr.structs["PlbLayerOutputs"]] == ["hidden_states", "attentions"]
    assert [n for n, _ in _lib.PlbLayerOutputs._fields_] == ["hidden_states", "attentions"]
    p = c_header.c_params(hdr, "plb_encode_bwd_layers")
    assert p[-3:] == ["const float* d_hidden", "const float* const* d_below", "void* stream"]
    assert c_header.c_params(hdr, "plb_encode_layers")[:-2] == c_header.c_params(hdr, "plb_encode")[:-1]
    assert c_header.c_params(khdr, "plb_launch_add_row_grad")[2:-2] == c_header.c_params(khdr, "plb_launch_seed_dy")[1:-2]
    from plbert_amd import build
    assert "layer_outputs.hip" in build.SOURCES
