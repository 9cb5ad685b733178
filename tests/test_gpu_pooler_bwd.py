"""plb_encode_bwd_pooled through the engine (-m gpu; include/plbert.h): the pooler backward composed with the encoder's, the
pooler range of the gradient buffer, the NULL form, the refusals, accumulation, the fused optimizers and the exchange.

Shapes. (P) the small_h128 fixture: H = 128, 2 heads, L = 2, B = 3, S = 40, lengths 40 / 33 / 7 — one 128-row tile, padded.
(K) the ragged shape of tests/test_gpu_encode.py that packs: B = 5, S = 300, lengths 300 / 129 / 128 / 65 / 1.

Composition is checked bit for bit, not to a tolerance: encode_bwd(G, d_pooled=P) must leave the encoder range that
encode_bwd(G') leaves, G' = G with the launcher's dh0 added (one torch fp32 add) to position 0 of every sample — the seed launch
makes the same add and the same rounding, and nothing else in the backward differs."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_cfg, load_golden
from gpu_util import rel_l2, stream
from pooler_gpu import POOL_B, POOL_W, launcher as _launcher
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import HipEngine, packing_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_SHAPE = (5, 300, [300, 129, 128, 65, 1])


def _err():
    return _lib.lib().plb_last_error().decode()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _case_p(num_tokens=0):
    g = load_golden("small_h128")
    ocfg, pcfg, sd = golden_cfg(g)
    B, S = g["labels"].shape
    eng = HipEngine(pcfg, int(g["num_phonemes"]), num_tokens, max_batch=B, max_seq=S)
    if num_tokens:
        sd = {**plbert_amd.deterministic_state_dict(pcfg, int(g["num_phonemes"]), num_tokens, seed=5), **sd}
    eng.load_state_dict(sd)
    return eng, np.asarray(g["masked"]), np.asarray(g["lengths"], np.int32), g


def _case_k():
    B, S, lengths = K_SHAPE
    pcfg = plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)
    rs = np.random.RandomState(100 * B + S)
    ids = np.zeros((B, S), np.int64)
    for b, n in enumerate(lengths):
        ids[b, :n] = rs.randint(1, 186, size=n)
    eng = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(pcfg, 188, seed=13))
    return eng, ids, np.asarray(lengths, np.int32)


def _ranges(eng):
    head0 = eng.layout["phoneme_predictor.weight"][0]
    pw, pb = eng.layout[POOL_W], eng.layout[POOL_B]
    assert eng.trainable == pw[0] and pw[0] + pw[1] == pb[0]
    return head0, pw[0], pb[0] + pb[1]


def _rand(shape, seed, scale=1e-2):
    return torch.as_tensor(np.random.RandomState(seed).randn(*shape) * scale, dtype=torch.float32).to(DEV)


def _compose(eng, ids, lens, G, P, packing=None, below=None, key_mask=None):
    """Returns (gradient buffer of the pooled call, of the composed call, the launcher's dW | db)."""
    hid = eng.encode(ids, lens, packing=packing, key_mask=key_mask)
    dwb, dh0 = _launcher(eng, hid, P)
    eng.grads.fill_(7.0)
    eng.encode_bwd(G, d_below=below, d_pooled=P)
    got = eng.grads.clone()
    hid2 = eng.encode(ids, lens, packing=packing, key_mask=key_mask)
    assert torch.equal(_bits(hid2), _bits(hid))
    G2 = torch.zeros_like(hid) if G is None else G.clone()
    G2[:, 0] = G2[:, 0] + dh0
    eng.grads.fill_(7.0)
    eng.encode_bwd(G2, d_below=below)
    return got, eng.grads.clone(), dwb


def _check_composition(eng, got, want, dwb):
    head0, p0, p1 = _ranges(eng)
    assert torch.equal(_bits(got[:head0]), _bits(want[:head0]))             # the encoder range, bit for bit
    assert float(got[:head0].abs().max()) > 0 and bool(torch.isfinite(got[:p1]).all())
    assert torch.equal(_bits(got[p0:p1]), _bits(dwb))                       # the pooler range IS the launcher's dW | db
    assert not bool(got[head0:p0].any())                                    # the head range: zeros
    assert bool((want[p0:p1] == 7.0).all()) and bool((got[p1:] == 7.0).all())   # without d_pooled the pooler range is not written


@pytest.mark.parametrize("variant", ["plain", "no_d_hidden", "d_below", "hole_at_0"])
def test_composition_padded(variant):
    eng, ids, lens, _ = _case_p()
    B, S, H = ids.shape[0], ids.shape[1], eng.cfg.hidden_size
    G, P = _rand((B, S, H), 1), _rand((B, H), 2, 1.0)
    below = key_mask = None
    if variant == "no_d_hidden":
        G = None
    if variant == "d_below":
        below = [None, _rand((B, S, H), 3)]
    if variant == "hole_at_0":
        key_mask = (torch.arange(S)[None, :] < torch.as_tensor(lens)[:, None]).int()
        key_mask[0, 0] = 0; key_mask[2, 0] = 0; key_mask[1, 5] = 0        # position 0 of samples 0 and 2 is a hole
    got, want, dwb = _compose(eng, ids, lens, G, P, below=below, key_mask=key_mask)
    _check_composition(eng, got, want, dwb)
    assert eng.status()["ln_exchange_timeouts"] == 0


@pytest.mark.parametrize("variant", ["plain", "no_d_hidden"])
def test_composition_packed(variant):
    eng, ids, lens = _case_k()
    B, S, H = ids.shape[0], ids.shape[1], eng.cfg.hidden_size
    plan = packing_plan(lens, S).to(DEV, non_blocking=False)
    assert plan.packed
    G = None if variant == "no_d_hidden" else _rand((B, S, H), 4)
    got, want, dwb = _compose(eng, ids, lens, G, _rand((B, H), 5, 1.0), packing=plan)
    _check_composition(eng, got, want, dwb)
    assert eng.last_call_rows() == (plan.rows, B * S)


def _raw_bwd(eng, name, ids_d, lens_d, B, S, d, d_pooled_ptr=None):
    args = [eng.handle, ids_d.data_ptr(), None, None, lens_d.data_ptr(), B, S, None, None if d is None else d.data_ptr(), None, None]
    if name == "plb_encode_bwd_pooled":
        args.append(d_pooled_ptr)
    return getattr(eng.L, name)(*args, stream())


def test_null_d_pooled_is_the_namesake_bit_for_bit_with_the_same_launches():
    eng, ids, lens, _ = _case_p()
    B, S = ids.shape
    G = _rand((B, S, eng.cfg.hidden_size), 6)
    eng._ensure_synced()
    ids_d, lens_d = eng._dev_i64(ids), eng._dev_i32(lens)
    out = []
    for name in ("plb_encode_bwd_masked", "plb_encode_bwd_pooled"):
        eng.encode(ids, lens)
        eng.grads.fill_(7.0)
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        _lib.profile_read()
        assert _raw_bwd(eng, name, ids_d, lens_d, B, S, G) == 0, _err()
        torch.cuda.synchronize()
        prof = _lib.profile_read()
        _lib.profile_enable(False)
        out.append((eng.grads.clone(), {k: v["launches"] for k, v in prof.items()}))
        # the engine state afterwards: the step that follows leaves the pooler (and the head) alone
        assert len(eng.adamw_plan(1, [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)], [0] * _lib.PLB_NPARAM)) >= 1
        assert max(s["end"] for s in eng.adamw_plan(1, [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)],
                                                    [0] * _lib.PLB_NPARAM)) == eng.layout["phoneme_predictor.weight"][0]
    assert torch.equal(_bits(out[0][0]), _bits(out[1][0]))
    assert out[0][1] == out[1][1] and sum(out[0][1].values()) > 10, out
    # with a d_pooled: exactly the two launch groups more (the pooler backward's three kernels, the seed of the first rows)
    eng.encode(ids, lens)
    P = _rand((B, eng.cfg.hidden_size), 7, 1.0)
    _lib.profile_enable(True)
    _lib.profile_read()
    assert _raw_bwd(eng, "plb_encode_bwd_pooled", ids_d, lens_d, B, S, G, P.data_ptr()) == 0, _err()
    torch.cuda.synchronize()
    prof = {k: v["launches"] for k, v in _lib.profile_read().items()}
    _lib.profile_enable(False)
    assert sum(prof.values()) == sum(out[0][1].values()) + 2, (prof, out[0][1])


def test_refusals_name_the_cause_and_launch_nothing():
    eng, ids, lens, g = _case_p(num_tokens=8)
    B, S, H = ids.shape[0], ids.shape[1], eng.cfg.hidden_size
    eng._ensure_synced()
    ids_d, lens_d = eng._dev_i64(ids), eng._dev_i32(lens)
    G, P = _rand((B, S, H), 8), _rand((B, H + 4), 9, 1.0).view(-1)
    eng.grads.copy_(torch.randn(eng.total, device=DEV))
    before = eng.grads.clone()

    def refused(rc, *words):
        assert rc != 0
        msg = _err()
        assert all(w in msg for w in words), msg
        torch.cuda.synchronize()
        assert torch.equal(_bits(eng.grads), _bits(before)), msg

    pooled = lambda d, p: _raw_bwd(eng, "plb_encode_bwd_pooled", ids_d, lens_d, B, S, d, p)
    refused(pooled(G, P.data_ptr()), "plb_encode_bwd_pooled", "no live plb_encode stash")
    eng.encode(ids, lens)
    refused(pooled(None, None), "nothing to differentiate", "d_pooled")
    refused(pooled(G, P.data_ptr() + 4), "plb_encode_bwd_pooled", "d_pooled must be 16-byte aligned")
    assert pooled(None, P.data_ptr()) == 0, _err()                          # the stash survived the refused calls
    torch.cuda.synchronize()
    # a window that would hold the token head's and the pooler's gradients: refused before any launch, both orders
    labels, masked = np.asarray(g["labels"]), np.asarray(g["masked"])
    off, flat = plbert_amd.masked_indices_to_csr([list(map(int, x)) for x in g["index"]])
    tok = np.random.RandomState(5).randint(0, 8, size=labels.shape).astype(np.int64)

    def dual():
        eng.loss_fwd_bwd(masked, labels, lens, off, flat, int(off[-1]), token_ids=tok)

    def with_pooler():
        eng.encode(ids, lens)
        eng.encode_bwd(G, d_pooled=P[: B * H].view(B, H))

    for first, second in ((dual, with_pooler), (with_pooler, dual)):
        first()
        eng.grad_accum_add(eng.GRAD_FIRST)
        second()
        torch.cuda.synchronize()
        before, accum = eng.grads.clone(), eng._accum.clone()
        for phase in (eng.GRAD_ADD, eng.GRAD_LAST):
            refused(eng.L.plb_grad_accum_add(eng.handle, phase, None, stream()), "plb_grad_accum_add", "token head", "pooler")
            assert torch.equal(_bits(eng._accum), _bits(accum))
    assert eng.status()["ln_exchange_timeouts"] == 0


def _norm_of(eng, *ranges):
    return float(torch.cat([eng.grads[a:b] for a, b in ranges]).double().pow(2).sum().sqrt())


def test_accumulation_of_two_micro_steps_and_the_norm():
    eng, ids, lens, _ = _case_p()
    B, S, H = ids.shape[0], ids.shape[1], eng.cfg.hidden_size
    head0, p0, p1 = _ranges(eng)
    single = []
    for k in (0, 1):
        eng.encode(ids, lens)
        eng.encode_bwd(_rand((B, S, H), 10 + k), d_pooled=_rand((B, H), 20 + k, 1.0))
        single.append(eng.grads.clone())
    eng.encode(ids, lens)
    eng.encode_bwd(_rand((B, S, H), 10), d_pooled=_rand((B, H), 20, 1.0))
    eng.grad_accum_add(eng.GRAD_FIRST)
    eng.encode(ids, lens)
    eng.encode_bwd(_rand((B, S, H), 11), d_pooled=_rand((B, H), 21, 1.0))
    eng.grad_accum_add(eng.GRAD_LAST, want_partials=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(eng.grads[p0:p1]), _bits(single[0][p0:p1] + single[1][p0:p1]))
    assert torch.equal(_bits(eng.grads[:head0]), _bits(single[0][:head0] + single[1][:head0]))
    want = _norm_of(eng, (0, head0), (p0, p1))
    from_partials = float(eng.grad_norm(1.0, 0.0, have_partials=True)[0])
    one_pass = float(eng.grad_norm(1.0, 0.0)[0])
    print(f"norm over encoder + pooler: {from_partials!r} (LAST's partials) {one_pass!r} (one pass) want {want!r}")
    assert abs(from_partials - want) <= 1e-6 * want and abs(one_pass - want) <= 1e-6 * want
    assert want > (1 + 1e-4) * _norm_of(eng, (0, head0))                    # (the pooler's share is visible at this tolerance)
    # a window whose second micro-step has no d_pooled: the pooler range keeps the first one's gradient and stays live
    eng.encode(ids, lens)
    eng.encode_bwd(_rand((B, S, H), 10), d_pooled=_rand((B, H), 20, 1.0))
    eng.grad_accum_add(eng.GRAD_FIRST)
    eng.encode(ids, lens)
    eng.encode_bwd(_rand((B, S, H), 11))
    eng.grads[p0:p1].fill_(float("nan"))                                    # not produced by this micro-step: never read
    eng.grad_accum_add(eng.GRAD_LAST)
    torch.cuda.synchronize()
    assert torch.equal(_bits(eng.grads[p0:p1]), _bits(single[0][p0:p1]))
    plan = eng.adamw_plan(1, [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)], [0] * _lib.PLB_NPARAM)
    assert max(s["end"] for s in plan) == p1


def _bf16_copy(eng):
    return eng.workspace[: 2 * eng.total].view(torch.bfloat16)   # (the flat bf16 copy opens the workspace)


def _pooled_backward(eng, ids, lens, seed):
    B, S, H = ids.shape[0], ids.shape[1], eng.cfg.hidden_size
    eng.encode(ids, lens)
    eng.encode_bwd(_rand((B, S, H), seed), d_pooled=_rand((B, H), seed + 1, 1.0))


GROUP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


@pytest.mark.parametrize("entry", ["adamw", "clipped", "groups", "lamb"])
def test_fused_step_on_the_pooler_range_against_torch_adamw(entry):
    eng, ids, lens, _ = _case_p(num_tokens=8)
    head0, p0, p1 = _ranges(eng)
    end = eng.total
    _pooled_backward(eng, ids, lens, 30)
    wd = 0.0 if entry == "lamb" else 0.01     # (LAMB with adapt off and no decay IS Adam: the comparison torch offers)
    ref = torch.nn.Parameter(eng.params[p0:p1].clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=wd, eps=1e-8)
    ref.grad = eng.grads[p0:p1].clone()
    enc0 = eng.params[:head0].clone()
    rest = [t.clone() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq)]
    bf0 = _bf16_copy(eng).clone()
    everything = {n: 0 for n in eng.layout}
    if entry == "adamw":
        eng.adamw_step(1, lr=1e-3, weight_decay=wd)
    elif entry == "clipped":
        eng.adamw_step(1, lr=1e-3, weight_decay=wd, norm_buf=eng.grad_norm(1.0, 1e9))
    elif entry == "groups":
        eng.adamw_step_groups(1, [GROUP], everything)
    else:
        eng.lamb_step(1, [dict(GROUP, weight_decay=0.0, adapt=False)], everything)
    opt.step()
    torch.cuda.synchronize()
    got = eng.params[p0:p1]
    print(f"{entry}: pooler range rel L2 {rel_l2(got, ref.detach()):.3e}")
    assert rel_l2(got, ref.detach()) < 1e-6
    assert float((got - ref.detach()).abs().max()) < 1e-6 * float(ref.detach().abs().max()) + 1e-9
    assert rel_l2(eng.exp_avg[p0:p1], opt.state[ref]["exp_avg"]) < 1e-6
    assert rel_l2(eng.exp_avg_sq[p0:p1], opt.state[ref]["exp_avg_sq"]) < 1e-6
    assert torch.equal(_bf16_copy(eng)[p0:p1], got.to(torch.bfloat16))
    assert not torch.equal(eng.params[:head0], enc0)                        # the encoder stepped too
    for was, now in zip(rest + [bf0], (eng.params, eng.exp_avg, eng.exp_avg_sq, _bf16_copy(eng))):
        assert torch.equal(was[head0:p0].view(torch.uint8), now[head0:p0].contiguous().view(torch.uint8))   # the phoneme head
        assert torch.equal(was[p1:end].view(torch.uint8), now[p1:end].contiguous().view(torch.uint8))       # the token head
    if entry == "lamb":
        res = eng.lamb_buf[: 4 * _lib.PLB_NPARAM].view(_lib.PLB_NPARAM, 4)
        i = _lib.PLB_PARAM_NAMES.index(POOL_W)
        assert float(res[i, 3]) == 1.0 and float(res[i, 2]) == 1.0
        assert abs(float(res[i, 0]) - float(rest[0][p0:p0 + eng.layout[POOL_W][1]].double().norm())) < 1e-5 * float(res[i, 0])
        assert not bool(res[_lib.PLB_PARAM_NAMES.index("phoneme_predictor.weight")].any())
    # a backward without d_pooled: the pooler has no gradient again and the step leaves it bit-unchanged
    snap = [t[p0:p1].clone() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq, _bf16_copy(eng))]
    eng.encode(ids, lens)
    eng.encode_bwd(_rand((ids.shape[0], ids.shape[1], eng.cfg.hidden_size), 40))
    eng.adamw_step(2, lr=1e-3)
    torch.cuda.synchronize()
    for was, now in zip(snap, (eng.params, eng.exp_avg, eng.exp_avg_sq, _bf16_copy(eng))):
        assert torch.equal(was.view(torch.uint8), now[p0:p1].contiguous().view(torch.uint8))


@pytest.mark.parametrize("entry", ["groups", "lamb"])
def test_a_frozen_pooler_is_bit_unchanged(entry):
    eng, ids, lens, _ = _case_p()
    head0, p0, p1 = _ranges(eng)
    _pooled_backward(eng, ids, lens, 50)
    eng.exp_avg[p0:p1].fill_(0.25); eng.exp_avg_sq[p0:p1].fill_(0.5)
    snap = [t[p0:p1].clone() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq, _bf16_copy(eng))]
    enc0 = eng.params[:head0].clone()
    thawed = {n: 0 for n in eng.layout if n not in (POOL_W, POOL_B)}
    assert max(s["end"] for s in eng.adamw_plan(1, [GROUP], thawed)) == head0
    assert max(s["end"] for s in eng.adamw_plan(1, [GROUP], {n: 0 for n in eng.layout})) == p1
    if entry == "groups":
        nb = eng.grad_norm(1.0, 1e9, group_of=thawed)
        assert abs(float(nb[0]) - _norm_of(eng, (0, head0))) <= 1e-6 * float(nb[0])      # the frozen pooler is no part of the norm
        eng.adamw_step_groups(1, [GROUP], thawed)
    else:
        eng.lamb_step(1, [dict(GROUP, adapt=True)], thawed)
        assert not bool(eng.lamb_buf[: 4 * _lib.PLB_NPARAM].view(_lib.PLB_NPARAM, 4)[_lib.PLB_PARAM_NAMES.index(POOL_W)].any())
    torch.cuda.synchronize()
    for was, now in zip(snap, (eng.params, eng.exp_avg, eng.exp_avg_sq, _bf16_copy(eng))):
        assert torch.equal(was.view(torch.uint8), now[p0:p1].contiguous().view(torch.uint8))
    assert not torch.equal(eng.params[:head0], enc0)
    # one of the two tensors thawed: the other one stays
    _pooled_backward(eng, ids, lens, 52)
    only_bias = dict(thawed, **{POOL_B: 0})
    (eng.adamw_step_groups if entry == "groups" else eng.lamb_step)(2, [dict(GROUP, adapt=True)], only_bias)
    torch.cuda.synchronize()
    nw = eng.layout[POOL_W][1]
    assert torch.equal(snap[0][:nw].view(torch.uint8), eng.params[p0:p0 + nw].contiguous().view(torch.uint8))
    assert not torch.equal(snap[0][nw:], eng.params[p0 + nw:p1])


@pytest.mark.parametrize("overlap", [True, False])
def test_one_rank_communicator_same_gradients_and_the_grown_piece(overlap):
    eng, ids, lens, _ = _case_p()
    head0, p0, p1 = _ranges(eng)
    runs = {}
    for pooled in (False, True):
        B, S, H = ids.shape[0], ids.shape[1], eng.cfg.hidden_size
        G, P = _rand((B, S, H), 60), _rand((B, H), 61, 1.0)
        eng.encode(ids, lens)
        eng.encode_bwd(G, d_pooled=P if pooled else None)
        alone = eng.grads[:p1].clone()
        eng.comm_init(HipEngine.comm_unique_id(), 0, 1)
        try:
            eng.set_grad_overlap(overlap)
            eng.hb_audit(True)
            eng.encode(ids, lens)
            eng.encode_bwd(G, d_pooled=P if pooled else None)
            eng.allreduce_grads()
            torch.cuda.synchronize()
            rep = eng.hb_report()
            assert rep["violations"] == 0, rep
            runs[pooled] = eng.comm_pieces()
            upto = p1 if pooled else p0
            assert torch.equal(_bits(eng.grads[:upto]), _bits(alone[:upto]))
        finally:
            eng.hb_audit(False)
            eng.comm_destroy()
    (c0, f0), (c1, f1) = runs[False], runs[True]
    assert c0 == c1 == (10 if overlap else 1), runs                         # the number of collectives stays
    assert f0 == eng.trainable and f1 == f0 + (p1 - p0), runs               # ... the float count grows by the pooler's size
