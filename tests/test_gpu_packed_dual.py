"""Token-packed execution of DUAL-HEAD loss calls (include/plbert.h: plb_set_packed_dual, plb_loss_fwd_bwd_dual_packed) on
the GPU: the two row kernels of the packed token head against a numpy restatement and the padded launch, the packed call
against the fp32 oracle and against the padded call of the same engine, the calls that stay padded, independence of what an
earlier call left in the workspace, and the trainer's switch.

Shapes (plans from plb_packing_plan; between them every branch of the token head's row handling):
  (5, 300, [300,129,128,65,1])   1024 used / 1024 rows of 1536: 256-row tiles, no tail, a one-token sample, a slot exactly full
  (6, 200, [200,127,64,13,1,1])   896 used / 1024 rows of 1280: 256-row tiles, a 128-row tail that no sample owns
  (2, 512, [512,300]) (fixture)   896 used /  896 rows of 1024: Tp % 256 != 0, the 128 x 256 tile form
Vocabularies: 1000 token classes (padded to 1024 columns) and 300 with the fixture's batch."""
import functools

import numpy as np
import pytest
import torch

from conftest import golden_cfg, load_golden
from gpu_util import assert_same_bits, rel_l2, stream
from oracle import albert_np as onp
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import HipEngine, packing_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY_BIAS = "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.key.bias"
# name: (B, S, lengths, num_tokens, used, rows, padded rows)
SHAPES = {
    "no_tail": (5, 300, [300, 129, 128, 65, 1], 1000, 1024, 1024, 1536),
    "tail": (6, 200, [200, 127, 64, 13, 1, 1], 1000, 896, 1024, 1280),
    "fixture": (2, 512, [512, 300], 300, 896, 896, 1024),
}
NAMES = list(SHAPES)


def _plan(lengths, S):
    plan = packing_plan(lengths, S).to(DEV, non_blocking=False)
    assert plan.packed
    return plan


def _shape_plan(name):
    B, S, lengths, NT, used, rows, padded = SHAPES[name]
    plan = _plan(lengths, S)
    assert (plan.used, plan.rows, (B * S + 127) // 128 * 128) == (used, rows, padded)
    return plan


def _row_index(plan):
    """(packed row, padded row) of every valid token, and the mask of packed rows that hold no token."""
    pr, dr = [], []
    for b in range(plan.B):
        n = int(min(max(plan.lengths[b], 1), plan.S))
        pr.append(torch.arange(n) + int(plan.row_start_host[b]))
        dr.append(torch.arange(n) + b * plan.S)
    pr, dr = torch.cat(pr).to(DEV), torch.cat(dr).to(DEV)
    hole = torch.ones(plan.rows, dtype=torch.bool, device=DEV)
    hole[pr] = False
    return pr, dr, hole


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("name", NAMES)
def test_pack_token_targets_kernel(name):
    """out[row_start[b] + s] = token_ids[b, s] for s < len_b, 0 on every other row, exactly; the pad positions of the input
    hold -1 and NT + 5 (never read: neither may appear), the output is prefilled with a sentinel (none may survive)."""
    L = _lib.lib()
    B, S, lengths, NT, used, rows, _ = SHAPES[name]
    plan = _shape_plan(name)
    rs = np.random.RandomState(11)
    tok = rs.randint(1, NT, size=(B, S)).astype(np.int64)
    valid = np.arange(S)[None, :] < np.asarray(lengths)[:, None]
    tok[~valid] = np.where(rs.rand(B, S) < 0.5, -1, NT + 5)[~valid]
    want = np.zeros(rows, np.int64)
    for b, n in enumerate(lengths):
        want[plan.row_start_host[b]: plan.row_start_host[b] + n] = tok[b, :n]
    sentinel = -(1 << 40) - 7
    out = torch.full((rows + 16,), sentinel, dtype=torch.int64, device=DEV)
    tok_d = torch.as_tensor(tok).to(DEV)
    lens_d = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    assert L.plb_launch_pack_token_targets(tok_d.data_ptr(), lens_d.data_ptr(), plan.row_start.data_ptr(), B, S, rows,
                                           out.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:rows], want)
    assert not np.isin(got[:rows], [sentinel, -1, NT + 5]).any()
    assert (got[rows:] == sentinel).all()                      # nothing behind the plan's rows is written
    # arguments the launcher refuses: a row count that is no plan's, a missing table, an output that is not 16-byte aligned
    bad = [(rows - 1, plan.row_start.data_ptr(), out.data_ptr()), (rows, None, out.data_ptr()),
           (rows, plan.row_start.data_ptr(), out.data_ptr() + 8)]
    for r, rsp, o in bad:
        assert L.plb_launch_pack_token_targets(tok_d.data_ptr(), lens_d.data_ptr(), rsp, B, S, r, o, stream()) != 0


@pytest.mark.parametrize("ntiles", [4, 250])
@pytest.mark.parametrize("name", NAMES)
def test_token_ce_combine_packed_kernel_is_bit_equal_to_the_padded_launch(name, ntiles):
    """The same per-token (max, sum) pairs and target logits in the padded and in the packed arrangement: lse, w and the
    loss row of every valid token are the same bits, every slot-pad and tail row is exactly 0.0 (outputs prefilled with
    NaN). 4 tiles: lanes without a tile; 250: lanes with three and four."""
    L = _lib.lib()
    B, S, lengths, NT, used, rows, padded = SHAPES[name]
    plan = _shape_plan(name)
    pr, dr, hole = _row_index(plan)
    g = torch.Generator().manual_seed(17 + ntiles)
    pmax0 = (torch.randn(padded, ntiles, generator=g) * 5).to(DEV)
    psum0 = (torch.rand(padded, ntiles, generator=g) * 200 + 0.5).to(DEV)
    tl0 = (torch.randn(padded, generator=g) * 5).to(DEV)
    pmax1 = torch.full((rows, ntiles), 3.0, device=DEV)
    psum1 = torch.full((rows, ntiles), 7.0, device=DEV)
    tl1 = torch.full((rows,), -2.0, device=DEV)
    pmax1[pr], psum1[pr], tl1[pr] = pmax0[dr], psum0[dr], tl0[dr]
    lens_d = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    nan = float("nan")
    o0 = [torch.full((padded,), nan, device=DEV) for _ in range(3)]
    o1 = [torch.full((rows,), nan, device=DEV) for _ in range(3)]
    assert L.plb_launch_token_ce_combine(pmax0.data_ptr(), psum0.data_ptr(), ntiles, tl0.data_ptr(), lens_d.data_ptr(), B, S,
                                         padded, o0[0].data_ptr(), o0[1].data_ptr(), o0[2].data_ptr(), stream()) == 0
    assert L.plb_launch_token_ce_combine_packed(pmax1.data_ptr(), psum1.data_ptr(), ntiles, tl1.data_ptr(), lens_d.data_ptr(),
                                                plan.row_start.data_ptr(), B, S, rows, o1[0].data_ptr(), o1[1].data_ptr(),
                                                o1[2].data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    for what, a, b in zip(("lse", "w", "loss_rows"), o1, o0):
        assert bool(torch.isfinite(b[dr]).all()), what
        assert torch.equal(a[pr].view(torch.int32), b[dr].view(torch.int32)), what
        assert int(hole.sum()) == rows - sum(lengths) and bool((a[hole].view(torch.int32) == 0).all()), what   # +0.0, no NaN left
    wb = torch.cat([torch.full((n,), 1.0 / (B * n)) for n in lengths]).to(DEV)
    assert torch.allclose(o1[1][pr], wb, rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------- engine
def _small_cfg(NT):
    pcfg = plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)
    ocfg = onp.Config(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2, intermediate_size=256,
                      num_hidden_layers=2, max_position_embeddings=512, num_phonemes=188, num_tokens=NT)
    return pcfg, ocfg


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs of one shape at the small config (that of test_dual_against_oracle), made once and left unchanged: seeded ids
    (the fixture's batch for the third shape), token targets, one sample with an empty index list."""
    B, S, lengths, NT, *_ = SHAPES[name]
    rs = np.random.RandomState(100 * B + S)
    if name == "fixture":
        g = load_golden("real_s512_b2_ragged")
        assert [int(x) for x in g["lengths"]] == lengths
        labels, masked = np.asarray(g["labels"], np.int64), np.asarray(g["masked"], np.int64)
        idx = [list(map(int, x)) for x in g["index"]]
        idx[1] = []
    else:
        labels, masked, idx = np.zeros((B, S), np.int64), np.zeros((B, S), np.int64), []
        for b, n in enumerate(lengths):
            labels[b, :n] = rs.randint(1, 185, size=n)
            masked[b, :n] = labels[b, :n]
            ii = sorted(rs.choice(n, size=max(1, n // 6), replace=False).tolist()) if b != 3 else []
            masked[b, ii] = 185
            idx.append(ii)
    tok = rs.randint(0, NT, size=(B, S)).astype(np.int64)
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    pcfg, ocfg = _small_cfg(NT)
    sd = plbert_amd.deterministic_state_dict(pcfg, 188, NT, seed=5)
    return dict(B=B, S=S, NT=NT, lengths=lengths, lens=np.asarray(lengths, np.int32), labels=labels, masked=masked, idx=idx,
                tok=tok, off=off, flat=flat, n=int(off[-1]), pcfg=pcfg, ocfg=ocfg, sd=sd)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    c = _case(name)
    loss, _, G = onp.loss_and_grads(c["ocfg"], c["sd"], c["masked"], c["labels"], c["lengths"], c["idx"], token_ids=c["tok"])
    return float(loss), G


def _engine(c, max_batch=None, max_seq=None, dual=None):
    eng = HipEngine(c["pcfg"], 188, c["NT"], max_batch=max_batch or c["B"], max_seq=max_seq or c["S"])
    eng.load_state_dict(c["sd"])
    if dual is not None:
        eng.set_packed_dual(dual)
    return eng


def _call(eng, c, plan=None, backward=True, n_masked=None):
    off, flat, n = (c["off"], c["flat"], c["n"]) if n_masked is None else (np.zeros_like(c["off"]), c["flat"][:0], 0)
    fn = eng.loss_fwd_bwd if backward else eng.loss_fwd
    loss = fn(c["masked"], c["labels"], c["lens"], off, flat, n, token_ids=c["tok"], packing=plan)
    torch.cuda.synchronize()
    return float(loss.item()), eng.loss_parts.clone()


@pytest.mark.parametrize("name", NAMES)
def test_packed_dual_against_oracle(name):
    """Bars of test_dual_against_oracle: loss 1e-3 relative, the tensors it checks 4e-2 relative L2; the call reports the
    plan's rows (a build that ignored the plan would report B*S) and loss_parts sums to the loss."""
    c = _case(name)
    loss_ref, G = _oracle(name)
    plan = _shape_plan(name)
    eng = _engine(c, dual=True)
    loss, parts = _call(eng, c, plan)
    assert eng.last_call_rows() == (plan.rows, c["B"] * c["S"]) and plan.rows < c["B"] * c["S"]
    assert eng.last_application_rows() == (plan.rows, plan.rows)          # a dual-head call prunes nothing
    print("loss", loss, "oracle", loss_ref, "parts", parts.tolist())
    assert abs(loss - loss_ref) / loss_ref < 1e-3
    assert abs(float(parts.double().sum()) - loss) <= 1e-6 * loss and float(parts[1]) > 0
    for k in ("token_predictor.weight", "token_predictor.bias", "phoneme_predictor.weight",
              "encoder.encoder.albert_layer_groups.0.albert_layers.0.ffn.weight",
              "encoder.embeddings.word_embeddings.weight"):
        err = rel_l2(eng.view(k, of=eng.grads).cpu(), torch.from_numpy(G[k]))
        print(k, err)
        assert err < 4e-2, (k, err)
    assert eng.status()["ln_exchange_timeouts"] == 0


def _compare_grads(eng, g_pk, g_pad, skip=()):
    for k, (o, sz, shp) in eng.layout.items():
        trainable = o + sz <= eng.trainable or k.startswith("token_predictor.")
        if not trainable or k == KEY_BIAS or k in skip:
            continue
        err = rel_l2(g_pk[o:o + sz], g_pad[o:o + sz])
        assert err < 1.5e-2, (k, err)


@pytest.mark.parametrize("name", NAMES)
def test_packed_dual_equals_padded_as_two_bf16_evaluations(name):
    """One engine, packed against padded — the bars of test_packed_equals_padded_as_two_bf16_evaluations: loss and both
    loss parts 1e-4 relative, every trainable tensor and the token head's 1.5e-2 relative L2 (its exclusion kept: the key
    bias, whose gradient is exactly zero). The loss-only call with the plan gives the packed training call's loss and
    parts bit for bit."""
    c = _case(name)
    plan = _shape_plan(name)
    eng = _engine(c, dual=True)
    l_pad, p_pad = _call(eng, c)
    assert eng.last_call_rows() == (c["B"] * c["S"],) * 2
    g_pad = eng.grads.clone()
    l_val, p_val = _call(eng, c, plan, backward=False)
    assert eng.last_call_rows() == (plan.rows, c["B"] * c["S"])
    l_pk, p_pk = _call(eng, c, plan)
    assert eng.last_call_rows() == (plan.rows, c["B"] * c["S"])
    g_pk = eng.grads.clone()
    assert l_val == l_pk and torch.equal(p_val, p_pk)
    print("loss packed", l_pk, "padded", l_pad, "parts", p_pk.tolist(), p_pad.tolist())
    assert abs(l_pk - l_pad) <= 1e-4 * l_pad
    for i in range(2):
        assert abs(float(p_pk[i]) - float(p_pad[i])) <= 1e-4 * float(p_pad[i]), i
    _compare_grads(eng, g_pk, g_pad)
    assert eng.status()["ln_exchange_timeouts"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_packed_dual_without_masked_positions(name):
    """n_masked == 0 with token targets: phoneme part 0.0, phoneme-head gradients exactly 0, the token term still trains —
    token and encoder gradients within the packed-against-padded bar of the padded call's."""
    c = _case(name)
    plan = _shape_plan(name)
    eng = _engine(c, dual=True)
    l_pad, p_pad = _call(eng, c, n_masked=0)
    g_pad = eng.grads.clone()
    eng.grads.fill_(1.0)
    l_pk, p_pk = _call(eng, c, plan, n_masked=0)
    g_pk = eng.grads.clone()
    assert eng.last_call_rows() == (plan.rows, c["B"] * c["S"])
    assert float(p_pk[0]) == 0.0 and l_pk == float(p_pk[1]) and abs(l_pk - l_pad) <= 1e-4 * l_pad
    heads = ("phoneme_predictor.weight", "phoneme_predictor.bias")
    for k in heads:
        assert float(eng.view(k, of=g_pk).abs().max()) == 0.0, k
    _compare_grads(eng, g_pk, g_pad, skip=heads)
    assert eng.status()["ln_exchange_timeouts"] == 0


def test_switch_off_runs_padded_bit_for_bit_and_token_logits_stay_padded():
    """Switch off (the default): plb_loss_fwd_bwd_dual_packed with a plan that packs gives plb_loss_fwd_bwd_dual's loss,
    parts and whole gradient buffer bit for bit and reports rows == B*S. Switch on: plb_forward_packed with token logits
    stays padded (fp8 mode: the next test)."""
    c = _case("fixture")
    B, S = c["B"], c["S"]
    plan = _shape_plan("fixture")
    eng = _engine(c)
    assert eng.packed_dual is False
    eng.grads.fill_(3.0)                       # (both calls start from the same buffer: the pooler's range is written by neither)
    l0, p0 = _call(eng, c)                     # plb_loss_fwd_bwd_dual
    g0 = eng.grads.clone()
    eng.grads.fill_(3.0)
    l1, p1 = _call(eng, c, plan)               # plb_loss_fwd_bwd_dual_packed, switch off
    assert eng.last_call_rows() == (B * S, B * S)
    assert l1 == l0 and torch.equal(p1, p0)
    assert_same_bits(eng, eng.grads, g0, "gradients of the new entry point with the switch off")
    # the switch turns it on and off again
    eng.set_packed_dual(True)
    _call(eng, c, plan)
    assert eng.last_call_rows() == (plan.rows, B * S)
    _, ph0, tk0 = eng.forward(c["masked"], c["lens"], want_token=True)
    _, ph1, tk1 = eng.forward(c["masked"], c["lens"], want_token=True, packing=plan)
    assert eng.last_call_rows() == (B * S, B * S)
    assert torch.equal(ph0, ph1) and torch.equal(tk0, tk1)
    eng.set_packed_dual(False)
    _call(eng, c, plan)
    assert eng.last_call_rows() == (B * S, B * S)
    assert eng.status()["ln_exchange_timeouts"] == 0


def test_fp8_dual_calls_run_padded_with_the_switch_on():
    """fp8 mode needs hidden size 768: the fixture's own model with a token head of 300 classes. Switch on, a plan that
    packs: the calibration call and the fp8 calls report rows == B*S and give the loss, parts and whole gradient buffer of
    the calls without a plan bit for bit."""
    c = dict(_case("fixture"))
    g = load_golden("real_s512_b2_ragged")
    _, c["pcfg"], _ = golden_cfg(g)
    c["sd"] = plbert_amd.reference_init_state_dict(c["pcfg"], 188, c["NT"], seed=0)
    B, S = c["B"], c["S"]
    plan = _shape_plan("fixture")
    res = []
    for pk in (None, plan):
        e8 = _engine(c, dual=True)
        e8.set_fp8(True)
        out = [_call(e8, c, pk) for _ in range(3)]
        assert e8.last_call_rows() == (B * S, B * S) and e8.fp8_state() == (True, True)
        res.append((out, e8.grads.clone()))
        assert e8.status()["ln_exchange_timeouts"] == 0
    for (la, pa), (lb, pb) in zip(res[0][0], res[1][0]):
        assert la == lb and torch.equal(pa, pb)
    assert_same_bits(e8, res[1][1], res[0][1], "fp8-mode gradients with and without a plan")


@pytest.mark.parametrize("name", NAMES)
def test_packed_dual_call_after_a_larger_padded_call_equals_a_fresh_engine(name):
    """Rows of the packed axis that hold no token (slot ends; for "tail" 128 rows that no sample owns) keep what a larger
    call left in the workspace: the token head's logit-gradient rows there must be written as zeros and its operands be
    finite, or the weight-gradient sums differ. Bit-identical loss and gradients to the same call on a fresh engine."""
    c = _case(name)
    B, S = c["B"], c["S"]
    plan = _shape_plan(name)
    fresh = _engine(c, max_batch=B + 2, dual=True)
    l0, p0 = _call(fresh, c, plan)
    g0 = fresh.grads.clone()
    used = _engine(c, max_batch=B + 2, dual=True)
    big_labels, big_masked, _, big_idx = plbert_amd.synthetic_batch(B + 2, S, seed=77)
    boff, bflat = plbert_amd.masked_indices_to_csr(big_idx)
    big_tok = np.random.RandomState(5).randint(0, c["NT"], size=(B + 2, S)).astype(np.int64)
    used.loss_fwd_bwd(big_masked, big_labels, None, boff, bflat, int(boff[-1]), token_ids=big_tok)
    assert used.last_call_rows() == ((B + 2) * S,) * 2
    l1, p1 = _call(used, c, plan)
    assert used.last_call_rows() == (plan.rows, B * S)
    assert l1 == l0 and torch.equal(p1, p0)
    assert_same_bits(used, used.grads, g0, "gradients of a packed dual-head call after a larger padded one")
    assert used.status()["ln_exchange_timeouts"] == 0


def test_trainer_packed_dual_switch():
    """PLBertTrainer(num_tokens=300, packed=True, packed_dual=...) on the ragged fixture: on, the dual-head step runs the
    plan's 896 rows and the loss falls over three steps; off, the same trainer runs 1,024."""
    from plbert_amd.train import PLBertTrainer
    g = load_golden("real_s512_b2_ragged")
    _, pcfg, _ = golden_cfg(g)
    idx = [list(map(int, x)) for x in g["index"]]
    lengths = [int(x) for x in g["lengths"]]
    tok = np.random.RandomState(1).randint(0, 300, size=g["labels"].shape).astype(np.int64)
    rows = {}
    for dual in (True, False):
        tr = PLBertTrainer(pcfg, int(g["num_phonemes"]), max_batch=2, max_seq=512, lr=7e-5, device=DEV, num_tokens=300,
                           packed=True, packed_dual=dual)
        assert tr.packed_dual is dual
        batch = tr.stage_batch(g["labels"], g["masked"], lengths, idx, token_ids=tok)
        assert batch.packing is not None and batch.packing.rows == 896
        losses = [float(tr.step(batch).item()) for _ in range(3 if dual else 1)]
        rows[dual] = tr.engine.last_call_rows()
        if dual:
            print("losses", losses)
            assert losses[2] < losses[1] < losses[0]
        assert tr.engine.status()["ln_exchange_timeouts"] == 0
    assert rows[True] == (896, 1024) and rows[False] == (1024, 1024)
