"""-m gpu: per-application outputs and their gradients through HipEngine (include/plbert.h: plb_forward_layers,
plb_encode_layers, plb_encode_bwd_layers).

Shapes (tests/test_gpu_encode.py): (P) the small_h128 fixture — H 128, 2 heads, L 2, B 3, S 40, lengths 40 / 33 / 7;
(K) B 5, S 300, lengths 300 / 129 / 128 / 65 / 1, packed, here with L = 3 (the shared layer's weights do not depend on L).

Gradients are checked against the UNCHANGED float64 oracle through the identity tests/test_layer_outputs_host.py proves:
the parameter gradient of sum_l <G_l, hidden_states[l]> is sum_l encoder_backward(l applications, caches[:l], G_l).

Attention maps against the oracle's `pr`. The fixtures' maps are nearly flat (heads differ by 3e-4 on (P), applications by
2e-4 on (K): checked on the CPU), so query.weight and key.weight of that test's state dict are scaled by 8 (SHARPEN). On (K)
applications 1 and 2 would still see nearly the same input (the hidden state moves by 7 % per application, their maps
differ by 7 times the bf16 error at any sharpness), so dense.weight and ffn_output.weight are scaled by 8 there as well: the
hidden state then moves by a third per application. The error of a map grows with its sharpness — application 0, whose
input no attention has shaped, is flat (largest probability 0.02) and 100 times closer to the oracle than the later ones —
so every application is held to twice ITS OWN measured worst max-abs (ATT_MEASURED, MI355X), which is never looser than one
figure per case, and the test asserts on the oracle's own values that the two heads of an application differ by more than
ten times that application's bound, and the maps of two applications by more than ten times the larger of their two
bounds: a mis-wired layer or head cannot pass. Oracle figures at these settings (max-abs): heads of application 0 / 1 (/ 2)
differ by 1.99e-2 / 0.983 on (P), 5.18e-3 / 0.993 / 0.969 on (K); applications by 0.946 on (P), 0.973 / 0.960 / 0.720 on (K)."""
import ctypes as C

import numpy as np
import pytest
import torch

import layer_outputs_ref as lref
from gpu_util import rel_l2, stream
from oracle import albert_np as onp
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import HipEngine
from test_gpu_encode import KEY_BIAS, K_SHAPE, _case_p, _check_against_oracle, _dh, _plan, _valid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYER = onp.LAYER
SHARPEN = {"P": (8.0, 1.0), "K": (8.0, 8.0)}   # case -> factors of (query.weight, key.weight), (dense.weight, ffn_output.weight)
# worst max-abs difference between attentions[l] and the oracle's map, per application, measured on MI355X with SHARPEN
ATT_MEASURED = {"P": (1.648e-04, 1.083e-02), "K": (2.651e-05, 1.642e-02, 1.667e-02)}


def _err():
    return _lib.lib().plb_last_error().decode()


def _k_cfg(L):
    return plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=L, max_position_embeddings=512)


def _case_k3(L=3, train=True, sd=None):
    """(K) of tests/test_gpu_encode.py with L applications."""
    B, S, lengths = K_SHAPE
    ocfg = onp.Config(embedding_size=64, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=L)
    pcfg = _k_cfg(L)
    sd = sd or plbert_amd.deterministic_state_dict(pcfg, 188, seed=13)
    rs = np.random.RandomState(100 * B + S)
    ids = np.zeros((B, S), np.int64)
    for b, n in enumerate(lengths):
        ids[b, :n] = rs.randint(1, 186, size=n)
    eng = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S, train=train)
    eng.load_state_dict(sd)
    return eng, ocfg, sd, ids, np.asarray(lengths, np.int32)


def _case(case, **kw):
    return _case_p()[:5] if case == "P" else _case_k3(**kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_pads_zero(hs, at, lens, S):
    v = torch.as_tensor(_valid(lens, S)).to(DEV)
    for h in hs:
        if h is not None:
            assert not bool(_bits(h[~v]).any())
    for a in at:
        if a is not None:
            assert not bool(_bits(a)[(~v)[:, None, :, None].expand_as(a)].any())     # pad query rows
            assert not bool(_bits(a)[(~v)[:, None, None, :].expand_as(a)].any())     # pad key columns


_ORACLE = {}


def _oracle_forward(case, ocfg, sd, ids, lens):
    """(hidden states [L+1], attention maps [L]) of the float64 oracle and its caches: computed once, shared, never modified."""
    if case not in _ORACLE:
        hid, caches = onp.encoder_forward(ocfg, sd, ids, onp.attention_mask_from_lengths(np.asarray(lens)), np.float64)
        _ORACLE[case] = (lref.hidden_states_of(hid, caches), [c["pr"] for c in caches["layers"]], caches)
    return _ORACLE[case]


# ---- forward: hidden states ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["P", "K"])
def test_last_slot_is_the_hidden_of_forward_and_pads_are_zero(case):
    eng, ocfg, sd, ids, lens = _case(case)
    B, S = ids.shape
    nl = eng.cfg.num_hidden_layers
    plan = _plan(lens, S) if case == "K" else None
    v = torch.as_tensor(_valid(lens, S)).to(DEV)
    want, _, _ = eng.forward(ids, lens, want_hidden=True, want_phoneme=False, packing=plan)
    hs, at, hid = eng.forward_layers(ids, lens, packing=plan, hidden_states=True, attentions=True, want_hidden=True)
    assert len(hs) == nl + 1 and len(at) == nl and all(t is not None for t in hs + at)
    assert eng.last_call_rows() == ((plan.rows, B * S) if plan is not None else (B * S, B * S))
    assert torch.equal(_bits(hid), _bits(want))                              # plb_forward_packed(hidden) as it always was
    assert torch.equal(_bits(hs[nl][v]), _bits(want[v]))
    _assert_pads_zero(hs, at, lens, S)
    for a in at:
        assert float((a.double().sum(-1)[v[:, None, :].expand(a.shape[:3])] - 1).abs().max()) <= 3e-3
    assert eng.status()["ln_exchange_timeouts"] == 0


def test_inner_slots_are_the_last_hidden_state_of_shallower_engines():
    eng, ocfg, sd, ids, lens = _case_k3()
    B, S = ids.shape
    plan = _plan(lens, S)
    v = torch.as_tensor(_valid(lens, S)).to(DEV)
    hs, _ = eng.forward_layers(ids, lens, packing=plan)
    for l in (1, 2):
        shallow = HipEngine(_k_cfg(l), 188, 0, max_batch=B, max_seq=S, train=False)
        shallow.load_state_dict(sd)
        want, _, _ = shallow.forward(ids, lens, want_hidden=True, want_phoneme=False, packing=plan)
        assert torch.equal(_bits(hs[l][v]), _bits(want[v])), l
        assert not torch.equal(_bits(hs[l][v]), _bits(hs[l + 1][v]))


def test_hidden_states_against_the_oracle():
    """Every slot of (P) within the bounds tests/test_gpu_engine.py holds `hidden` to: max-abs 6e-2, rel-L2 1e-2 (valid positions)."""
    eng, ocfg, sd, ids, lens = _case_p()[:5]
    B, S = ids.shape
    ref_hs, _, _ = _oracle_forward("P", ocfg, sd, ids, lens)
    v = _valid(lens, S)
    hs, _ = eng.forward_layers(ids, lens)
    assert len(hs) == len(ref_hs) == eng.cfg.num_hidden_layers + 1
    for l, (got, ref) in enumerate(zip(hs, ref_hs)):
        g, r = got.cpu().double()[torch.as_tensor(v)], torch.as_tensor(ref)[torch.as_tensor(v)]
        print(f"hidden_states[{l}]: max-abs {float((g - r).abs().max()):.3e} rel-L2 {rel_l2(g, r):.3e}")
        assert float((g - r).abs().max()) < 6e-2 and rel_l2(g, r) < 1e-2, l


def test_packed_equals_padded_on_every_output():
    eng, ocfg, sd, ids, lens = _case_k3()
    B, S = ids.shape
    v = torch.as_tensor(_valid(lens, S)).to(DEV)
    hs_pad, at_pad = eng.forward_layers(ids, lens, hidden_states=True, attentions=True)
    assert eng.last_call_rows() == (B * S, B * S)
    plan = _plan(lens, S)
    hs_pk, at_pk = eng.forward_layers(ids, lens, packing=plan, hidden_states=True, attentions=True)
    assert eng.last_call_rows() == (plan.rows, B * S)
    for a, b in zip(hs_pad, hs_pk):
        assert torch.equal(_bits(a[v]), _bits(b[v]))
    for a, b in zip(at_pad, at_pk):
        assert torch.equal(_bits(a), _bits(b))          # valid rows bit-equal; everything else is zero in both (below)
    _assert_pads_zero(hs_pad, at_pad, lens, S)
    _assert_pads_zero(hs_pk, at_pk, lens, S)


# ---- forward: attention maps -----------------------------------------------------------------------------------------------
def _sharpened(sd, case):
    qk, mix = SHARPEN[case]
    out = dict(sd)
    for n, f in (("attention.query", qk), ("attention.key", qk), ("attention.dense", mix), ("ffn_output", mix)):
        k = LAYER + n + ".weight"
        out[k] = torch.as_tensor(np.asarray(sd[k])) * f
    return out


@pytest.mark.parametrize("case", ["P", "K"])
def test_attentions_against_the_oracle(case):
    eng, ocfg, sd, ids, lens = _case(case)
    B, S = ids.shape
    sd = _sharpened(sd, case)
    eng.load_state_dict(sd)
    _, ref_at, _ = _oracle_forward(case + "-sharp", ocfg, sd, ids, lens)
    plan = _plan(lens, S) if case == "K" else None
    _, at = eng.forward_layers(ids, lens, packing=plan, hidden_states=False, attentions=True)
    rows = torch.as_tensor(_valid(lens, S))[:, None, :, None]
    bound = [2 * m for m in ATT_MEASURED[case]]
    assert len(bound) == len(at) == len(ref_at)
    ref = [torch.as_tensor(r) * rows for r in ref_at]
    worst = []
    for l, got in enumerate(at):
        worst.append(float((got.cpu().double() * rows - ref[l]).abs().max()))
        heads = float((ref[l][:, 0] - ref[l][:, 1]).abs().max())
        print(f"attentions[{l}] ({case}): max-abs to the oracle {worst[l]:.3e} (bound {bound[l]:.3e}); the oracle's heads differ by {heads:.3e}")
        assert heads > 10 * bound[l], (l, heads, bound[l])
        for j in range(l):
            apps = float((ref[l] - ref[j]).abs().max())
            print(f"    the oracle's applications {j} and {l} differ by {apps:.3e}")
            assert apps > 10 * max(bound[l], bound[j]), (j, l, apps, bound)
    assert all(w < b for w, b in zip(worst, bound)), (worst, bound)


# ---- encode(layers=...), subsets, inference-only, fp8 --------------------------------------------------------------------
@pytest.mark.parametrize("case", ["P", "K"])
def test_encode_layers_equals_forward_layers(case):
    eng, ocfg, sd, ids, lens = _case(case)
    B, S = ids.shape
    plan = _plan(lens, S) if case == "K" else None
    hs, at = eng.forward_layers(ids, lens, packing=plan, hidden_states=True, attentions=True)
    plain = eng.encode(ids, lens, packing=plan)
    hid, ehs, eat = eng.encode(ids, lens, packing=plan, layers=dict(hidden_states=True, attentions=True))
    assert torch.equal(_bits(hid), _bits(plain)) and torch.equal(_bits(hid), _bits(ehs[-1]))
    for a, b in zip(hs + at, ehs + eat):
        assert torch.equal(_bits(a), _bits(b))
    # layers given, nothing asked for: plb_encode itself, and its stash is live
    hid2, ehs2, eat2 = eng.encode(ids, lens, packing=plan, layers=dict())
    assert torch.equal(_bits(hid2), _bits(plain)) and not any(t is not None for t in ehs2 + eat2)
    eng.encode_bwd(torch.zeros_like(hid2))


def test_a_subset_of_slots_writes_only_those():
    eng, ocfg, sd, ids, lens = _case_k3()
    B, S = ids.shape
    nl, H, NH = 3, 128, 2
    plan = _plan(lens, S)
    hs, at = eng.forward_layers(ids, lens, packing=plan, hidden_states=True, attentions=True)
    all_hs = [torch.full((B, S, H), -7.0, device=DEV) for _ in range(nl + 1)]
    all_at = [torch.full((B, NH, S, S), -7.0, device=DEV) for _ in range(nl)]
    pick_h, pick_a = (0, 2), (1,)
    eng.forward_layers(ids, lens, packing=plan, out=([t if i in pick_h else None for i, t in enumerate(all_hs)],
                                                     [t if i in pick_a else None for i, t in enumerate(all_at)]))
    torch.cuda.synchronize()
    for i, (t, want) in enumerate(zip(all_hs, hs)):
        assert torch.equal(_bits(t), _bits(want)) if i in pick_h else bool((t == -7.0).all()), i
    for i, (t, want) in enumerate(zip(all_at, at)):
        assert torch.equal(_bits(t), _bits(want)) if i in pick_a else bool((t == -7.0).all()), i
    # the allocating form: None in the slots not asked for, negative indices count from the end
    hs2, at2 = eng.forward_layers(ids, lens, packing=plan, hidden_states=[-1, 1], attentions=[0])
    assert [t is not None for t in hs2] == [False, True, False, True] and [t is not None for t in at2] == [True, False, False]
    assert torch.equal(_bits(hs2[1]), _bits(hs[1])) and torch.equal(_bits(hs2[3]), _bits(hs[3])) and torch.equal(_bits(at2[0]), _bits(at[0]))
    with pytest.raises(ValueError, match="slot outside"):
        eng.forward_layers(ids, lens, hidden_states=[4])


def test_inference_only_engine_gives_the_same_bits():
    eng, ocfg, sd, ids, lens = _case_k3()
    inf = _case_k3(train=False)[0]
    plan = _plan(lens, ids.shape[1])
    for packing in (None, plan):
        a = eng.forward_layers(ids, lens, packing=packing, hidden_states=True, attentions=True)
        b = inf.forward_layers(ids, lens, packing=packing, hidden_states=True, attentions=True)
        for x, y in zip(a[0] + a[1], b[0] + b[1]):
            assert torch.equal(_bits(x), _bits(y))


def test_forward_layers_in_fp8_mode():
    """Two engines with one call history (fp8 on, the calibration call, then the call under test): the last slot of
    forward_layers is the hidden of forward in that mode, bit for bit, and the maps are probabilities."""
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  num_hidden_layers=2, max_position_embeddings=512)
    sd = plbert_amd.deterministic_state_dict(cfg, 188, seed=3)
    B, S, lens = 2, 128, np.asarray([128, 77], np.int32)
    ids = np.random.RandomState(0).randint(1, 180, size=(B, S))
    ids[1, 77:] = 0
    v = torch.as_tensor(_valid(lens, S)).to(DEV)
    engs = []
    for _ in range(2):
        e = HipEngine(cfg, 188, 0, max_batch=B, max_seq=S, train=False)
        e.load_state_dict(sd)
        e.set_fp8(True)
        e.forward(ids, lens, want_hidden=True, want_phoneme=False)      # calibrates in bf16
        engs.append(e)
    assert engs[0].fp8_state()[0]
    want, _, _ = engs[0].forward(ids, lens, want_hidden=True, want_phoneme=False)
    hs, at, hid = engs[1].forward_layers(ids, lens, hidden_states=True, attentions=True, want_hidden=True)
    assert torch.equal(_bits(hid), _bits(want)) and torch.equal(_bits(hs[-1][v]), _bits(want[v]))
    _assert_pads_zero(hs, at, lens, S)
    for a in at:
        assert float((a.double().sum(-1)[v[:, None, :].expand(a.shape[:3])] - 1).abs().max()) <= 3e-3
    assert engs[0].fp8_state() == engs[1].fp8_state()


# ---- launches ---------------------------------------------------------------------------------------------------------------
def _launches(fn):
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    try:
        _lib.profile_read()
        fn()
        torch.cuda.synchronize()
        return {k: v["launches"] for k, v in _lib.profile_read().items()}
    finally:
        _lib.profile_enable(False)


def test_calls_that_ask_for_nothing_launch_what_they_launched():
    """Per kernel class (the comparison of tests/test_gpu_grad_accum.py): forward, encode and encode_bwd launch the same on a
    fresh engine and on one that has used every new entry point; a layers call that asks for nothing launches what its
    namesake launches; one that asks launches exactly one conversion pass per hidden state (cast_transpose), one probability
    launch per map and one row-add per gradient slot (gather_scatter_rows) more. An all-NULL d_below leaves the gradient
    buffer of plb_encode_bwd, bit for bit."""
    fresh, ocfg, sd, ids, lens = _case_k3()
    used = _case_k3()[0]
    B, S = ids.shape
    plan = _plan(lens, S)
    d = torch.as_tensor(_dh((B, S, 128), _valid(lens, S), 5), dtype=torch.float32, device=DEV)
    used.forward_layers(ids, lens, packing=plan, hidden_states=True, attentions=True)
    used.encode(ids, lens, packing=plan, layers=dict(hidden_states=True, attentions=True))
    used.encode_bwd(None, d_below=[d, None, d])
    calls = {
        "forward": lambda e: e.forward(ids, lens, want_hidden=True, want_phoneme=False, packing=plan),
        "encode": lambda e: e.encode(ids, lens, packing=plan),
        "encode_bwd": lambda e: e.encode_bwd(d),
    }
    for e in (fresh, used):   # warm: weight copies in place
        e.forward(ids, lens, packing=plan)
    base = {}
    for name, fn in calls.items():
        a, b = _launches(lambda: fn(fresh)), _launches(lambda: fn(used))
        assert a == b and sum(a.values()) > 0, (name, a, b)
        base[name] = a
    g_plain = used.grads.clone()
    nothing = _launches(lambda: used.forward_layers(ids, lens, packing=plan, hidden_states=False, attentions=False, want_hidden=True))
    assert nothing == base["forward"]
    assert _launches(lambda: used.encode(ids, lens, packing=plan, layers=dict())) == base["encode"]
    assert _launches(lambda: used.encode_bwd(d, d_below=[None] * 3)) == base["encode_bwd"]
    assert torch.equal(_bits(used.grads), _bits(g_plain))

    def plus(counts, **more):
        out = dict(counts)
        for k, n in more.items():
            out[k] = out.get(k, 0) + n
        return out

    got = _launches(lambda: used.forward_layers(ids, lens, packing=plan, hidden_states=[0, 2], attentions=[1], want_hidden=True))
    assert got == plus(base["forward"], cast_transpose=2, gather_scatter_rows=1), (got, base["forward"])
    got = _launches(lambda: used.encode(ids, lens, packing=plan, layers=dict(hidden_states=True, attentions=True)))
    assert got == plus(base["encode"], cast_transpose=4, gather_scatter_rows=3), (got, base["encode"])
    got = _launches(lambda: used.encode_bwd(d, d_below=[d, None, d]))
    assert got == plus(base["encode_bwd"], gather_scatter_rows=2), (got, base["encode_bwd"])
    assert used.status()["ln_exchange_timeouts"] == 0


# ---- gradients --------------------------------------------------------------------------------------------------------------
def _slot_gradients(B, S, H, lens, nl, seed):
    """G_l ~ N(0, 1e-2) at valid positions, 0 at pads (float64, for the oracle), and what goes to the device: NaN at pads."""
    v = _valid(lens, S)
    G = [_dh((B, S, H), v, seed + l) for l in range(nl + 1)]
    dev = []
    for g in G:
        t = torch.as_tensor(g, dtype=torch.float32)
        t[torch.as_tensor(~v)] = float("nan")
        dev.append(t.to(DEV))
    return G, dev


@pytest.mark.parametrize("case", ["P", "K"])
@pytest.mark.parametrize("slots", ["all", "inner"])
def test_layer_gradients_against_the_oracle(case, slots):
    eng, ocfg, sd, ids, lens = _case(case)
    B, S = ids.shape
    nl, H = eng.cfg.num_hidden_layers, eng.cfg.hidden_size
    _, _, caches = _oracle_forward(case, ocfg, sd, ids, lens)
    G, dev = _slot_gradients(B, S, H, lens, nl, 40)
    inner = nl - 1                                            # (P): slot 1 of 0..2, (K): slot 2 of 0..3
    if slots == "inner":
        G = [g if l == inner else None for l, g in enumerate(G)]
        dev = [g if l == inner else None for l, g in enumerate(dev)]
    want = lref.layer_gradient_sum(ocfg, sd, caches, G)
    assert set(want) == {k for k in eng.layout if k.startswith("encoder.") and "pooler" not in k}
    plan = _plan(lens, S) if case == "K" else None
    eng.grads.fill_(7.0)                                      # overwritten, not accumulated
    eng.encode(ids, lens, packing=plan)
    eng.encode_bwd(dev[nl], d_below=dev[:nl])                 # ("inner": d_hidden is None)
    torch.cuda.synchronize()
    _check_against_oracle(eng, want)
    assert eng.status()["ln_exchange_timeouts"] == 0


def test_packed_layer_gradients_equal_padded():
    """(K), packing on against off with gradients at every slot: the bound of test_packed_encode_bwd_equals_padded."""
    eng, ocfg, sd, ids, lens = _case_k3()
    B, S = ids.shape
    _, dev = _slot_gradients(B, S, 128, lens, 3, 50)
    eng.encode(ids, lens)
    eng.encode_bwd(dev[3], d_below=dev[:3])
    g_pad = eng.grads[: eng.trainable].clone()
    plan = _plan(lens, S)
    eng.encode(ids, lens, packing=plan)
    eng.encode_bwd(dev[3], d_below=dev[:3])
    assert eng.last_call_rows() == (plan.rows, B * S)
    g_pk = eng.grads[: eng.trainable].clone()
    head0 = eng.layout["phoneme_predictor.weight"][0]
    for k, (o, sz, shp) in eng.layout.items():
        if o + sz > head0 or k == KEY_BIAS:
            continue
        r = rel_l2(g_pk[o:o + sz], g_pad[o:o + sz])
        print(f"{k}: packed vs padded rel L2 {r:.3e}")
        assert r < 1.5e-2, (k, r)


# ---- call-history independence ------------------------------------------------------------------------------------------------
def test_layers_calls_do_not_depend_on_the_call_history():
    fresh, ocfg, sd, ids, lens = _case_k3()
    used = _case_k3()[0]
    B, S = ids.shape
    plan = _plan(lens, S)
    _, dev = _slot_gradients(B, S, 128, lens, 3, 60)
    # a loss call (padded, then packed) and a report on the used engine
    rs = np.random.RandomState(4)
    labels = rs.randint(1, 186, size=(B, S)).astype(np.int64)
    idx = [sorted(rs.choice(int(n), size=max(1, int(n) // 7), replace=False).tolist()) for n in lens]
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    used.loss_fwd_bwd(ids, labels, lens, off, flat, int(off[-1]))
    used.loss_fwd_bwd(ids, labels, lens, off, flat, int(off[-1]), packing=plan)
    used.masked_report(torch.as_tensor(off).to(DEV), want=("totals",))
    used.forward(ids, lens, packing=plan)
    out = []
    for e in (fresh, used):
        hs, at = e.forward_layers(ids, lens, packing=plan, hidden_states=True, attentions=True)
        hid, ehs, eat = e.encode(ids, lens, packing=plan, layers=dict(hidden_states=True, attentions=True))
        e.encode_bwd(dev[3], d_below=dev[:3])
        torch.cuda.synchronize()
        out.append(hs + at + [hid] + ehs + eat + [e.grads[: e.trainable].clone()])
        assert e.status()["ln_exchange_timeouts"] == 0
    for a, b in zip(*out):
        assert torch.equal(_bits(a), _bits(b))


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause_and_launch_nothing():
    eng, ocfg, sd, ids, lens = _case_k3()
    B, S = ids.shape
    L, h = eng.L, eng.handle
    unbound = HipEngine(_k_cfg(3), 188, 0, max_batch=B, max_seq=S)             # created, never bound
    eng._ensure_synced()
    ids_d, lens_d = eng._dev_i64(ids), eng._dev_i32(lens)
    hid = torch.full((B, S, 128), -7.0, device=DEV)
    slots = [torch.full((B, S, 128), -7.0, device=DEV) for _ in range(4)]
    maps = [torch.full((B, 2, S, S), -7.0, device=DEV) for _ in range(3)]
    lo, keep = eng._layer_outputs(slots, maps, B, S)
    d = torch.zeros((B, S, 128), device=DEV)
    eng.grads.copy_(torch.randn(eng.total, device=DEV))
    before = eng.grads.clone()

    def fwd(handle=h, ids_p=ids_d.data_ptr(), B_=B, fn=None):
        return (fn or L.plb_forward_layers)(handle, ids_p, lens_d.data_ptr(), B_, S, None, hid.data_ptr(), C.byref(lo), stream())

    def bwd(handle=h, d_hidden=None, below=None, B_=B):
        arr = None if below is None else (C.c_void_p * 3)(*below)
        return L.plb_encode_bwd_layers(handle, ids_d.data_ptr(), lens_d.data_ptr(), B_, S, None, d_hidden,
                                       None if arr is None else C.addressof(arr), stream())

    def refused(rc, who, *words):
        assert rc != 0
        msg = _err()
        assert msg.startswith(who + ":") and all(w in msg for w in words), msg
        torch.cuda.synchronize()
        assert torch.equal(_bits(eng.grads), _bits(before)), msg
        assert all(bool((t == -7.0).all()) for t in [hid] + slots + maps), msg

    refused(fwd(handle=None), "plb_forward_layers", "engine not bound")
    refused(fwd(handle=unbound.handle), "plb_forward_layers", "engine not bound")
    refused(fwd(ids_p=None), "plb_forward_layers", "ids is null")
    refused(fwd(B_=B + 1), "plb_forward_layers", "exceeds the engine capacity")
    enc = L.plb_encode_layers
    refused(fwd(handle=None, fn=enc), "plb_encode_layers", "engine not bound")
    refused(fwd(handle=unbound.handle, fn=enc), "plb_encode_layers", "engine not bound")
    refused(fwd(ids_p=None, fn=enc), "plb_encode_layers", "ids is null")
    refused(enc(h, ids_d.data_ptr(), lens_d.data_ptr(), B, S, None, None, C.byref(lo), stream()), "plb_encode_layers", "hidden is null")
    inf = _case_k3(train=False)[0]
    inf._ensure_synced()
    refused(fwd(handle=inf.handle, fn=enc), "plb_encode_layers", "inference-only")
    refused(bwd(handle=None, d_hidden=d.data_ptr()), "plb_encode_bwd_layers", "engine not bound")
    refused(bwd(handle=unbound.handle, d_hidden=d.data_ptr()), "plb_encode_bwd_layers", "engine not bound")
    refused(bwd(handle=inf.handle, d_hidden=d.data_ptr()), "plb_encode_bwd_layers", "inference-only")
    refused(bwd(d_hidden=d.data_ptr()), "plb_encode_bwd_layers", "no live plb_encode stash")
    eng.encode(ids, lens)                                                      # a live stash from here on
    refused(bwd(), "plb_encode_bwd_layers", "nothing to differentiate")
    refused(bwd(below=[None, None, None]), "plb_encode_bwd_layers", "nothing to differentiate")
    refused(bwd(d_hidden=d.data_ptr(), B_=B - 1), "plb_encode_bwd_layers", "differs", f"batch {B - 1} x seq {S}")
    plan = _plan(lens, S)
    pk = plan.c_struct(eng.device)
    refused(L.plb_encode_bwd_layers(h, ids_d.data_ptr(), lens_d.data_ptr(), B, S, C.byref(pk), d.data_ptr(), None, stream()),
            "plb_encode_bwd_layers", "packing plan differs")
    assert bwd(below=[None, d.data_ptr(), None]) == 0, _err()                  # the stash survived every refused call
    torch.cuda.synchronize()
    before = eng.grads.clone()
    refused(bwd(d_hidden=d.data_ptr()), "plb_encode_bwd_layers", "no live plb_encode stash", "has consumed it")
    # fp8 mode: plb_encode_layers refuses as plb_encode does
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  num_hidden_layers=1, max_position_embeddings=512)
    e8 = HipEngine(cfg, 188, 0, max_batch=1, max_seq=128)
    e8.load_state_dict(plbert_amd.deterministic_state_dict(cfg, 188, seed=3))
    e8.set_fp8(True)
    with pytest.raises(RuntimeError, match="plb_encode_layers.*fp8 mode is on"):
        e8.encode(np.random.RandomState(0).randint(1, 180, size=(1, 128)), layers=dict(hidden_states=True))
    del keep


def test_happens_before_audit_with_an_inner_slot():
    eng, ocfg, sd, ids, lens = _case_k3()
    B, S = ids.shape
    plan = _plan(lens, S)
    _, dev = _slot_gradients(B, S, 128, lens, 3, 70)
    eng._bind()
    eng.hb_audit(True)
    eng.encode(ids, lens, packing=plan, layers=dict(hidden_states=True, attentions=True))
    eng.encode_bwd(None, d_below=[None, dev[1], None])
    torch.cuda.synchronize()
    rep = eng.hb_report()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep
    eng.hb_audit(False)
