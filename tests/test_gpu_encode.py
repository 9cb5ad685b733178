"""The differentiable encoder through the C ABI (-m gpu; include/plbert.h: plb_encode / plb_encode_bwd): the seed kernel bit
for bit, the forward against plb_forward, the gradients against the float64 oracle (oracle.albert_np.encoder_backward),
against this library's own loss call and between the packed and the padded layout, the life of the stash, the optimizer
range, the happens-before audit and the exchange at world size 2.

Shapes. (P) the small_h128 fixture's own config, weights and batch: H = 128, 2 heads, L = 2, B = 3, S = 40, lengths
40 / 33 / 7 — T = 120, Tp = 128, the smallest the kernels accept. (K) one of the ragged shapes of tests/test_gpu_packed.py
that actually pack: B = 5, S = 300, lengths 300 / 129 / 128 / 65 / 1 — a full sample, one that crosses a 128-row boundary by
one row, samples shorter than a slot."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden_cfg, load_golden
from gpu_util import rel_l2, stream
from oracle import albert_np as onp
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import HipEngine, packing_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_BIAS = "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.key.bias"
QUERY_BIAS = KEY_BIAS.replace("key", "query")
K_SHAPE = (5, 300, [300, 129, 128, 65, 1])


def _err():
    return _lib.lib().plb_last_error().decode()


def _case_p():
    g = load_golden("small_h128")
    ocfg, pcfg, sd = golden_cfg(g)
    B, S = g["labels"].shape
    eng = HipEngine(pcfg, int(g["num_phonemes"]), 0, max_batch=B, max_seq=S)
    eng.load_state_dict(sd)
    return eng, ocfg, sd, np.asarray(g["masked"]), np.asarray(g["lengths"], np.int32), g


def _case_k():
    B, S, lengths = K_SHAPE
    ocfg = onp.Config(embedding_size=64, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2)
    pcfg = plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)
    sd = plbert_amd.deterministic_state_dict(pcfg, 188, seed=13)
    rs = np.random.RandomState(100 * B + S)
    ids = np.zeros((B, S), np.int64)
    for b, n in enumerate(lengths):
        ids[b, :n] = rs.randint(1, 186, size=n)
    eng = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S)
    eng.load_state_dict(sd)
    return eng, ocfg, sd, ids, np.asarray(lengths, np.int32)


def _plan(lens, S):
    plan = packing_plan(lens, S).to(DEV, non_blocking=False)
    assert plan.packed
    return plan


def _valid(lens, S):
    return np.arange(S)[None, :] < np.asarray(lens)[:, None]


def _dh(shape, valid, seed):
    """Upstream gradient: N(0, 1e-2) at valid positions, 0 at pads."""
    d = np.random.RandomState(seed).randn(*shape) * 1e-2
    d[~valid] = 0.0
    return d


# ---- seed kernel ------------------------------------------------------------------------------------------------------
def _seed_values(n, seed):
    """fp32 test values: seeded normals, +-0, subnormals, exact bf16 rounding midpoints of both parities, the largest
    finite values (they round to +-inf in bf16, as torch's conversion does)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 4)
    bits = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x807F8000,
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x42FE8000, 0x42FF8000, 0x3F808001, 0x3F807FFF,
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7E8000]
    special = torch.tensor(np.array(bits, dtype=np.uint32).view(np.float32))
    pos = torch.randperm(n, generator=g)[: 8 * len(bits)]
    x[pos] = special.repeat(8)
    return x


@pytest.mark.parametrize("case", ["P", "K", "H768"])
def test_seed_dy_is_bit_exact_and_writes_every_row_once(case):
    L = _lib.lib()
    if case == "P":
        B, S, H, lens, packed = 3, 40, 128, [40, 33, 7], False
    elif case == "K":
        (B, S, lens), H, packed = K_SHAPE, 128, True
    else:   # more than one block of the grid, H no power of two, a tail of 116 rows behind B*S
        B, S, H, lens, packed = 2, 70, 768, [70, 3], False
    lens = np.asarray(lens, np.int32)
    valid = torch.as_tensor(_valid(lens, S))
    d = _seed_values(B * S * H, 7).view(B, S, H)
    d[~valid] = float("nan")          # never read: a NaN that reached dy would show below
    d = d.to(DEV)
    lens_d = torch.as_tensor(lens).to(DEV)
    if packed:
        plan = _plan(lens, S)
        Tp, row_start = plan.rows, plan.row_start
        rows = torch.cat([torch.arange(int(n)) + int(plan.row_start_host[b]) for b, n in enumerate(lens)])
    else:
        Tp, row_start = (B * S + 127) // 128 * 128, None
        rows = torch.cat([torch.arange(int(n)) + b * S for b, n in enumerate(lens)])
    dy = torch.full((Tp + 8, H), -1.5, dtype=torch.bfloat16, device=DEV)   # sentinel (0xBFC0), 8 guard rows behind Tp
    sentinel = int(dy[0, 0].view(torch.int16))
    assert L.plb_launch_seed_dy(d.data_ptr(), lens_d.data_ptr(), None if row_start is None else row_start.data_ptr(), B, S, H,
                                Tp, dy.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    got = dy.cpu().view(torch.int16)
    want = d.cpu()[valid].to(torch.bfloat16).view(torch.int16)   # [valid tokens, H], in (b, s) order — as `rows`
    assert torch.equal(got[rows], want)
    other = torch.ones(Tp, dtype=torch.bool)
    other[rows] = False
    assert int(other.sum()) == Tp - int(lens.sum()) and not bool(got[:Tp][other].any())   # all-zero bytes
    # (so no sentinel survives in [0, Tp): every row there is either equal to the reference or zero bytes)
    assert bool((got[Tp:] == sentinel).all())                   # nothing behind row Tp was written
    # lengths == NULL (padded only): every position is valid
    if not packed:
        d2 = torch.nan_to_num(d, nan=0.25)
        assert L.plb_launch_seed_dy(d2.data_ptr(), None, None, B, S, H, Tp, dy.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(dy[: B * S].cpu().view(torch.int16), d2.cpu().view(B * S, H).to(torch.bfloat16).view(torch.int16))
        assert not bool(dy[B * S:Tp].cpu().view(torch.int16).any())
    # bad arguments are refused before any launch
    assert L.plb_launch_seed_dy(d.data_ptr(), lens_d.data_ptr(), None, B, S, H, B * S - 1, dy.data_ptr(), stream()) != 0
    assert L.plb_launch_seed_dy(d.data_ptr() + 4, lens_d.data_ptr(), None, B, S, H, Tp, dy.data_ptr(), stream()) != 0
    assert L.plb_launch_seed_dy(None, lens_d.data_ptr(), None, B, S, H, Tp, dy.data_ptr(), stream()) != 0


def test_unpack_rows_padded_layout_zeroes_the_pads():
    """plb_launch_unpack_rows with row_start == NULL: the conversion pass of a padded plb_encode."""
    L = _lib.lib()
    B, S, Cc, ld = 3, 40, 128, 136
    lens = torch.tensor([40, 33, 7], dtype=torch.int32, device=DEV)
    src = torch.randn(B * S, ld, device=DEV).to(torch.bfloat16)
    dst = torch.full((B, S, Cc), 9.0, device=DEV)
    assert L.plb_launch_unpack_rows(src.data_ptr(), 1, ld, None, lens.data_ptr(), B, S, Cc, dst.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    v = torch.as_tensor(_valid(lens.cpu().numpy(), S)).to(DEV)
    assert torch.equal(dst[v], src.view(B, S, ld)[..., :Cc].float()[v])
    assert float(dst[~v].abs().max()) == 0.0


# ---- forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["P", "K"])
def test_encode_hidden_equals_forward_and_is_zero_at_pads(case):
    eng, ocfg, sd, ids, lens = (_case_p() if case == "P" else _case_k())[:5]
    B, S = ids.shape
    plan = _plan(lens, S) if case == "K" else None
    want, _, _ = eng.forward(ids, lens, want_hidden=True, want_phoneme=False, packing=plan)
    got = eng.encode(ids, lens, packing=plan)
    rows, of = eng.last_call_rows()
    assert of == B * S and ((rows < of and rows == plan.rows) if plan is not None else rows == of)
    v = torch.as_tensor(_valid(lens, S)).to(DEV)
    assert torch.equal(got[v].view(torch.int32), want[v].view(torch.int32))
    assert not bool(got[~v].view(torch.int32).any())            # exactly +0.0
    if case == "K":   # the same shape in the padded layout: plb_forward's values, and zeros where it leaves whatever
        want_pad, _, _ = eng.forward(ids, lens, want_hidden=True, want_phoneme=False)
        got_pad = eng.encode(ids, lens)
        assert eng.last_call_rows() == (B * S, B * S)
        assert torch.equal(got_pad[v].view(torch.int32), want_pad[v].view(torch.int32))
        assert not bool(got_pad[~v].view(torch.int32).any())


# ---- gradients against the float64 oracle -----------------------------------------------------------------------------
_ORACLE = {}


def _oracle(case, ocfg, sd, ids, lens, dh):
    if case not in _ORACLE:   # computed once, shared, never modified
        am = onp.attention_mask_from_lengths(np.asarray(lens))
        _, caches = onp.encoder_forward(ocfg, sd, ids, am, np.float64)
        _ORACLE[case] = onp.encoder_backward(ocfg, sd, caches, dh.astype(np.float64), np.float64)
    return _ORACLE[case]


def _check_against_oracle(eng, G):
    """The bound of tests/test_gpu_engine.py::test_loss_and_grads_small for this fixture against the same oracle: per-tensor
    relative L2 4e-2; key bias (true gradient 0): norm below 2e-2 of the query-bias gradient's."""
    worst = {}
    for k, want in G.items():
        got = eng.view(k, of=eng.grads).cpu()
        if k == KEY_BIAS:
            scale = float(eng.view(QUERY_BIAS, of=eng.grads).double().norm())
            print(f"{k}: norm {float(got.double().norm()):.3e} vs query-bias norm {scale:.3e}")
            assert float(got.double().norm()) < 2e-2 * scale, (k, float(got.double().norm()), scale)
            continue
        want = torch.as_tensor(want)
        assert got.shape == want.shape
        worst[k] = rel_l2(got, want)
        print(f"{k}: rel L2 {worst[k]:.3e}")
    bad = {k: v for k, v in worst.items() if not v < 4e-2}
    assert not bad, bad
    head0 = eng.layout["phoneme_predictor.weight"][0]
    assert float(eng.grads[head0:eng.trainable].abs().max()) == 0.0 and eng.trainable > head0


@pytest.mark.parametrize("case", ["P", "K"])
def test_encode_bwd_gradients_against_the_oracle(case):
    eng, ocfg, sd, ids, lens = (_case_p() if case == "P" else _case_k())[:5]
    B, S = ids.shape
    H = eng.cfg.hidden_size
    dh = _dh((B, S, H), _valid(lens, S), 21)
    G = _oracle(case, ocfg, sd, ids, lens, dh)
    assert set(G) == {k for k in eng.layout if k.startswith("encoder.") and "pooler" not in k}
    plan = _plan(lens, S) if case == "K" else None
    eng.grads.fill_(7.0)                                      # overwritten, not accumulated
    eng.encode(ids, lens, packing=plan)
    d = torch.as_tensor(dh, dtype=torch.float32)
    d[torch.as_tensor(~_valid(lens, S))] = float("nan")       # pad positions of d_hidden are ignored
    eng.encode_bwd(d)
    torch.cuda.synchronize()
    if plan is not None:
        rows, of = eng.last_call_rows()
        assert rows < of and rows == plan.rows
    _check_against_oracle(eng, G)
    assert eng.status()["ln_exchange_timeouts"] == 0


def test_packed_encode_bwd_equals_padded():
    """(K), packing on against packing off: the bounds tests/test_gpu_packed.py sets between the packed and the padded loss
    call (two bf16 evaluations of one function): every tensor 1.5e-2 relative L2, the key bias left out.
    The packed call runs AFTER a padded one on the same engine, so rows of its token axis that hold no token carry what that
    call left: before the layer loop zeroed the dQKV slot of packed calls with S % 128 != 0 this test measured value.weight
    3.08e-2, map-in bias 1.42e-2, query.weight 1.3e-3, key.weight 7.8e-4 and every other tensor below 2e-7 (the attention
    backward stores no dK / dV row at or past position S, a full-length sample's slot runs on to the next multiple of 128)."""
    eng, ocfg, sd, ids, lens = _case_k()
    B, S = ids.shape
    d = torch.as_tensor(_dh((B, S, eng.cfg.hidden_size), _valid(lens, S), 22), dtype=torch.float32)
    eng.encode(ids, lens)
    eng.encode_bwd(d)
    assert eng.last_call_rows() == (B * S, B * S)
    g_pad = eng.grads[: eng.trainable].clone()
    plan = _plan(lens, S)
    eng.encode(ids, lens, packing=plan)
    eng.encode_bwd(d)
    assert eng.last_call_rows() == (plan.rows, B * S)
    g_pk = eng.grads[: eng.trainable].clone()
    head0 = eng.layout["phoneme_predictor.weight"][0]
    for k, (o, sz, shp) in eng.layout.items():
        if o + sz > head0 or k == KEY_BIAS:
            continue
        r = rel_l2(g_pk[o:o + sz], g_pad[o:o + sz])
        print(f"{k}: packed vs padded rel L2 {r:.3e}")
        assert r < 1.5e-2, (k, r)


# ---- two routes to one gradient -----------------------------------------------------------------------------------------
def _reference_loss_torch(logits, labels, lens, idx):
    """calculate_phoneme_loss (reference train.py:107-131): per-sample mean cross entropy over the masked positions, mean
    over the samples that have any."""
    total, count = 0.0, 0
    for b, ii in enumerate(idx):
        if len(ii):
            ii = torch.as_tensor(ii, device=logits.device)
            total = total + torch.nn.functional.cross_entropy(logits[b, :lens[b]][ii], labels[b, :lens[b]][ii])
            count += 1
    return total / count


# Measured on MI355X: the maximum per-tensor relative L2 between the two routes over the encoder tensors (key bias left
# out: its true gradient is 0), for the seeds 0 / 1 / 2 of the loss positions. The asserted bound is twice the largest and
# stays under the 4e-2 bound this fixture has against the oracle.
TWO_ROUTES_MEASURED = (6.5005e-03, 5.2796e-03, 5.7082e-03)
TWO_ROUTES_BOUND = 2 * max(TWO_ROUTES_MEASURED)   # 1.30e-2


def test_two_routes_to_one_gradient():
    """encode -> torch's gradient of the reference phoneme loss through the phoneme head -> encode_bwd, against
    loss_fwd_bwd of the same batch with the last application unpruned: two paths of this library to one gradient (they
    differ in where bf16 rounding happens: the loss call rounds the logit gradient and the head's dX GEMM output, this
    route rounds d_hidden once)."""
    eng, ocfg, sd, ids, lens, g = _case_p()
    B, S = ids.shape
    labels = np.asarray(g["labels"])
    Wp, bp = eng.view("phoneme_predictor.weight"), eng.view("phoneme_predictor.bias")
    head0 = eng.layout["phoneme_predictor.weight"][0]
    assert TWO_ROUTES_BOUND < 4e-2
    L = _lib.lib()
    worst_all = []
    try:
        L.plb_set_prune_last(0)
        for seed in (0, 1, 2):
            rs = np.random.RandomState(seed)
            # (the fixture's input ids; the seed draws the positions the loss reads)
            idx = [sorted(rs.choice(int(n), size=max(1, int(n) // 6), replace=False).tolist()) for n in lens]
            masked = ids
            off, flat = plbert_amd.masked_indices_to_csr(idx)
            eng.loss_fwd_bwd(masked, labels, lens, off, flat, int(off[-1]))
            assert eng.last_application_rows()[0] == eng.last_application_rows()[1]
            g_loss = eng.grads[:head0].clone()
            hid = eng.encode(masked, lens).requires_grad_(True)
            loss = _reference_loss_torch(hid @ Wp.T + bp, torch.as_tensor(labels).to(DEV), lens, idx)
            (d_hidden,) = torch.autograd.grad(loss, hid)
            eng.encode_bwd(d_hidden)
            g_enc = eng.grads[:head0].clone()
            worst = 0.0
            for k, (o, sz, shp) in eng.layout.items():
                if o + sz > head0 or k == KEY_BIAS:
                    continue
                worst = max(worst, rel_l2(g_enc[o:o + sz], g_loss[o:o + sz]))
            print(f"seed {seed}: max per-tensor rel L2 between the two routes {worst:.4e}")
            worst_all.append(worst)
    finally:
        L.plb_set_prune_last(-1)
    assert max(worst_all) < TWO_ROUTES_BOUND, worst_all


# ---- life of the stash --------------------------------------------------------------------------------------------------
def test_state_machine_failures_name_the_cause_and_leave_grads_alone():
    eng, ocfg, sd, ids, lens = _case_k()
    B, S = ids.shape
    H = eng.cfg.hidden_size
    L, h = eng.L, eng.handle
    eng._ensure_synced()
    ids_d, lens_d = eng._dev_i64(ids), eng._dev_i32(lens)
    d = torch.zeros((B, S, H), device=DEV)
    hid = torch.empty((B, S, H), device=DEV)
    plan = _plan(lens, S)
    pk = plan.c_struct(eng.device)
    eng.grads.copy_(torch.randn(eng.total, device=DEV))
    before = eng.grads.clone()

    def bwd(B_=B, S_=S, packing=None):
        return L.plb_encode_bwd(h, ids_d.data_ptr(), lens_d.data_ptr(), B_, S_, packing, d.data_ptr(), stream())

    def enc(packing=None):
        assert L.plb_encode(h, ids_d.data_ptr(), lens_d.data_ptr(), B, S, packing, hid.data_ptr(), stream()) == 0, _err()

    def refused(rc, *words):
        assert rc != 0
        msg = _err()
        assert msg.startswith("plb_encode") and all(w in msg for w in words), msg
        torch.cuda.synchronize()
        assert torch.equal(eng.grads.view(torch.int32), before.view(torch.int32)), msg

    refused(bwd(), "no live plb_encode stash", "no plb_encode has run")
    enc()
    eng.forward(ids, lens)
    refused(bwd(), "no live plb_encode stash", "plb_forward")
    enc()
    eng.adamw_step(1, lr=0.0, weight_decay=0.0)       # (lr 0: parameters stay; moments move, gradients are only read)
    refused(bwd(), "no live plb_encode stash", "plb_adamw_step")
    enc()
    refused(bwd(B_=B - 1), "differs", f"batch {B - 1} x seq {S}", f"{B} x {S}")
    refused(bwd(S_=S - 1), "differs", f"batch {B} x seq {S - 1}", f"{B} x {S}")
    refused(bwd(packing=C.byref(pk)), "packing plan differs")
    enc(C.byref(pk))
    refused(bwd(), "packing plan differs")
    assert bwd(packing=C.byref(pk)) == 0, _err()       # the stash survived the refused calls
    torch.cuda.synchronize()
    before = eng.grads.clone()
    refused(bwd(packing=C.byref(pk)), "no live plb_encode stash", "plb_encode_bwd has consumed it")
    # null arguments
    refused(L.plb_encode(h, None, lens_d.data_ptr(), B, S, None, hid.data_ptr(), stream()), "ids is null")
    refused(L.plb_encode(h, ids_d.data_ptr(), lens_d.data_ptr(), B, S, None, None, stream()), "hidden is null")
    # an inference-only engine keeps one layer of activations
    inf = HipEngine(eng.cfg, 188, 0, max_batch=B, max_seq=S, train=False)
    inf.load_state_dict(sd)
    inf._ensure_synced()
    refused(inf.L.plb_encode(inf.handle, ids_d.data_ptr(), lens_d.data_ptr(), B, S, None, hid.data_ptr(), stream()),
            "inference-only")
    with pytest.raises(RuntimeError, match="train=False"):
        inf.encode(ids, lens)


def test_encode_is_refused_in_fp8_mode():
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  num_hidden_layers=1, max_position_embeddings=512)
    eng = HipEngine(cfg, 188, 0, max_batch=1, max_seq=128)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(cfg, 188, seed=3))
    ids = np.random.RandomState(0).randint(1, 180, size=(1, 128))
    eng.set_fp8(True)
    before = eng.grads.clone()
    with pytest.raises(RuntimeError, match="fp8 mode is on"):
        eng.encode(ids)
    assert torch.equal(eng.grads, before)
    eng.set_fp8(False)
    hid = eng.encode(ids)                              # lengths == None: nothing is padded
    eng.set_fp8(False)                                 # ... and plb_set_fp8 ends the life of the stash
    with pytest.raises(RuntimeError, match="plb_set_fp8"):
        eng.encode_bwd(torch.zeros_like(hid))


def test_no_residue_in_the_next_loss_call():
    eng, ocfg, sd, ids, lens, g = _case_p()
    labels, masked = np.asarray(g["labels"]), np.asarray(g["masked"])
    off, flat = plbert_amd.masked_indices_to_csr([list(map(int, x)) for x in g["index"]])
    n = int(off[-1])
    l1 = eng.loss_fwd_bwd(masked, labels, lens, off, flat, n).clone()
    g1 = eng.grads.clone()
    hid = eng.encode(masked, lens)
    eng.encode_bwd(torch.randn_like(hid))
    assert not torch.equal(eng.grads[: eng.trainable], g1[: eng.trainable])
    l3 = eng.loss_fwd_bwd(masked, labels, lens, off, flat, n).clone()
    assert torch.equal(l3.view(torch.int32), l1.view(torch.int32))
    assert torch.equal(eng.grads.view(torch.int32), g1.view(torch.int32))


def test_adamw_after_encode_bwd_leaves_the_phoneme_head_alone():
    eng, ocfg, sd, ids, lens, g = _case_p()
    labels, masked = np.asarray(g["labels"]), np.asarray(g["masked"])
    off, flat = plbert_amd.masked_indices_to_csr([list(map(int, x)) for x in g["index"]])
    head0, end = eng.layout["phoneme_predictor.weight"][0], eng.trainable
    # a pre-training step first: the head's moments are non-zero, so an update with a zero gradient would move everything
    eng.loss_fwd_bwd(masked, labels, lens, off, flat, int(off[-1]))
    eng.adamw_step(1, lr=1e-3, weight_decay=0.01)
    bf16_copy = lambda: eng.workspace[: 2 * eng.total].view(torch.bfloat16)   # (the flat bf16 copy opens the workspace)
    assert torch.equal(bf16_copy()[:end], eng.params[:end].to(torch.bfloat16))
    snap = lambda t: t[head0:end].clone()
    p0, m0, v0, b0 = snap(eng.params), snap(eng.exp_avg), snap(eng.exp_avg_sq), snap(bf16_copy())
    assert float(m0.abs().max()) > 0
    hid = eng.encode(masked, lens)
    eng.encode_bwd(torch.randn_like(hid) * 1e-2)
    ref = torch.nn.Parameter(eng.params[:head0].clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=0.01)
    opt.state[ref] = {"step": torch.tensor(1.0), "exp_avg": eng.exp_avg[:head0].clone(),
                      "exp_avg_sq": eng.exp_avg_sq[:head0].clone()}
    ref.grad = eng.grads[:head0].clone()
    pool = eng.params[end:].clone()
    eng.adamw_step(2, lr=1e-3, weight_decay=0.01)
    opt.step()
    torch.cuda.synchronize()
    for was, now in ((p0, eng.params), (m0, eng.exp_avg), (v0, eng.exp_avg_sq), (b0, bf16_copy())):
        assert torch.equal(was.view(torch.uint8), now[head0:end].contiguous().view(torch.uint8))
    assert torch.equal(eng.params[end:], pool)
    # the encoder range: torch.optim.AdamW on a copy with the same gradients, the bound of tests/test_gpu_adamw_kernel.py
    assert rel_l2(eng.params[:head0], ref.detach()) < 1e-6
    assert float((eng.params[:head0] - ref.detach()).abs().max()) < 1e-6 * float(ref.detach().abs().max()) + 1e-9
    assert rel_l2(eng.exp_avg[:head0], opt.state[ref]["exp_avg"]) < 1e-6
    assert rel_l2(eng.exp_avg_sq[:head0], opt.state[ref]["exp_avg_sq"]) < 1e-6
    assert torch.equal(bf16_copy()[:head0], eng.params[:head0].to(torch.bfloat16))
    # the next loss call makes the head live again
    eng.loss_fwd_bwd(masked, labels, lens, off, flat, int(off[-1]))
    eng.adamw_step(3, lr=1e-3, weight_decay=0.01)
    assert not torch.equal(eng.params[head0:end], p0) and not torch.equal(eng.exp_avg[head0:end], m0)


def test_happens_before_audit_of_an_encode_pair():
    eng, ocfg, sd, ids, lens = _case_k()
    plan = _plan(lens, ids.shape[1])
    eng._bind()
    eng.hb_audit(True)
    hid = eng.encode(ids, lens, packing=plan)
    eng.encode_bwd(torch.randn_like(hid) * 1e-2)
    torch.cuda.synchronize()
    rep = eng.hb_report()
    assert rep["violations"] == 0 and rep["checks"] > 0, rep
    eng.hb_audit(False)


# ---- world size 2 through the stand-in RCCL -----------------------------------------------------------------------------
_WORLD2_WORKER = r"""
import ctypes as C, json, os, sys
rank, port, lib, out, root = int(sys.argv[1]), sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5]
sys.path.insert(0, root)
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, PLBERT_RCCL_LIB=lib, FAKE_RCCL_TIMEOUT_S="60")
import numpy as np, torch, torch.distributed as dist
dist.init_process_group("gloo", rank=rank, world_size=2)
import plbert_amd
from plbert_amd.engine import HipEngine
from plbert_amd.train import exchange_unique_id
torch.cuda.set_device(0)
cfg = plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                              intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)
B, S, H = 2, 64, 128
eng = HipEngine(cfg, 188, 0, max_batch=B, max_seq=S)
eng.load_state_dict(plbert_amd.deterministic_state_dict(cfg, 188, seed=13))
ids = np.random.RandomState(3).randint(1, 186, size=(B, S))
lens = np.asarray([64, 40], np.int32)
ids[1, 40:] = 0
dh = [torch.as_tensor(np.random.RandomState(10 + r).randn(B, S, H) * 1e-2, dtype=torch.float32) for r in (0, 1)]
n, head0 = eng.trainable, eng.layout["phoneme_predictor.weight"][0]
single = []
for r in (0, 1):   # the two single-rank results, no communicator
    eng.encode(ids, lens); eng.encode_bwd(dh[r])
    single.append(eng.grads[:n].clone())
want = single[0] + single[1]
res = {}
for overlap in (True, False):
    uid = exchange_unique_id(HipEngine.comm_unique_id if rank == 0 else None)
    eng.comm_init(uid, rank, 2)
    eng.set_grad_overlap(overlap)
    eng.hb_audit(True)
    eng.encode(ids, lens); eng.encode_bwd(dh[rank])
    issued = eng.comm_pieces()
    eng.allreduce_grads()
    torch.cuda.synchronize()
    rep = eng.hb_report()
    res["overlap" if overlap else "serial"] = dict(
        info=list(eng.comm_info()), issued=list(issued), pieces=list(eng.comm_pieces()),
        equal=bool(torch.equal(eng.grads[:n], want)), differs_from_own=not bool(torch.equal(eng.grads[:n], single[rank])),
        head_zero=float(eng.grads[head0:n].abs().max()) == 0.0, violations=rep["violations"], checks=rep["checks"],
        timeouts=eng.status()["ln_exchange_timeouts"])
    eng.hb_audit(False)
    eng.comm_destroy()
F = C.CDLL(lib)
F.fake_rccl_errors.restype = C.c_uint
res["fake_rccl_errors"] = int(F.fake_rccl_errors())
dist.barrier()
dist.destroy_process_group()
json.dump(res, open(out, "w"))
"""


def test_encode_bwd_world2_through_the_stand_in_rccl(fake_lib, tmp_path):
    """Two ranks, one GPU, tests/fake_rccl.cpp (the launcher of tests/test_gpu_comm_fake_rccl.py, as two child processes that
    each run under a time limit of their own): different d_hidden per rank; after plb_allreduce_grads every rank holds the
    sum of the two single-rank results — bit for bit, the bar that file sets for the loss call (a two-term fp32 sum has one
    order) — through the ten pieces of a regular step (overlap on) or one all-reduce (overlap off), and the stand-in saw
    the same collective sequence on both ranks."""
    port = str(29800 + (os.getpid() % 1500))
    outs = [str(tmp_path / f"rank{r}.json") for r in (0, 1)]
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, "-c", _WORLD2_WORKER, str(r), port, fake_lib,
                               outs[r], ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in (0, 1)]
    logs = [p.communicate()[0] for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} (exit {p.returncode}):\n{logs[r][-3000:]}"
    n_train = None
    for r in (0, 1):
        res = json.load(open(outs[r]))
        assert res["fake_rccl_errors"] == 0, "the stand-in saw mismatched collectives or a time-out"
        for key, pieces in (("overlap", 10), ("serial", 1)):
            got = res[key]
            assert got["info"] == [r, 2, 29999], got                      # the stand-in, not a real RCCL
            assert got["equal"] and got["differs_from_own"] and got["head_zero"], (r, key, got)
            assert got["pieces"][0] == pieces and got["violations"] == 0 and got["timeouts"] == 0, (r, key, got)
            assert got["issued"][0] == (10 if key == "overlap" else 0), (r, key, got)   # overlap: issued by plb_encode_bwd itself
            n_train = n_train or got["pieces"][1]
            assert got["pieces"][1] == n_train                              # the whole trainable range, on both ranks
        assert res["overlap"]["checks"] > 0 and res["serial"]["checks"] > 0, res   # (the audit saw cross-stream accesses)
