"""Gradient accumulation and global-norm clipping on the GPU (-m gpu): the kernels through their launchers, the engine's
window bookkeeping (ranges, liveness, misuse), the clipped AdamW against plb_adamw_step and torch.optim.AdamW, and
PLBertTrainer.step_accumulated against one step on the whole batch (include/plbert.h: plb_grad_accum_add, plb_grad_norm,
plb_adamw_step_clipped). Engine of tests/test_gpu_adamw_kernel.py: embedding 64, hidden 128, 2 heads, FFN 256, 2 layers,
max_batch 4, max_seq 32.

The norm tolerance. A partial sum is formed by one thread adding 4 squares per pass of its workgroup over its chunk (a
fused multiply-add each: one rounding), 6 steps of the wave reduction and 3 additions over the four waves:
_lib.norm_chain(n) = 4 * chunk(n) / 1024 + 6 + 3 fp32 additions at the most lie behind one partial (csrc/plbert_kernels.h:
PLB_NORM_CHAIN). All terms are non-negative, so each rounding is at most 2^-24 of the final partial: the sum of squares is
within (chain + 2) * 2^-24 relative of the float64 sum (the 2: the double sum over the partials and the result's rounding
to fp32), the norm within half of that."""
import numpy as np
import pytest
import torch

from gpu_util import assert_same_bits, rel_l2, stream
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import HipEngine
from plbert_amd.train import PLBertTrainer

pytestmark = pytest.mark.gpu

PARTS = _lib.PLB_NORM_PARTS
# 4 floats; a partial last pass; several workgroups and a tail; one workgroup's chunk and 4 floats of the next; the first
# size at which a chunk takes a second pass
SIZES = [4, 1020, 1024 * 7 + 4, 1024 + 4, PARTS * 1024 + 4]
GUARD = 64   # floats on either side of a range (the range stays 16-byte aligned)


def _cfg():
    return plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)


def _norm_bound(n):
    return 0.5 * (_lib.norm_chain(n) + 2) * 2.0 ** -24


def _wide(n, gen, zeros=True):
    """Gradients spanning many magnitudes, some exactly zero (tests/test_gpu_adamw_kernel.py)."""
    g = torch.randn(n, device="cuda", generator=gen) * torch.exp(torch.randn(n, device="cuda", generator=gen) * 3 - 6)
    if zeros:
        g[::97] = 0.0
    return g


def _guarded(n, fill=123.25):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill=123.25):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


def _finish(L, partials, nparts, grad_scale, max_norm, out):
    assert L.plb_launch_grad_norm_finish(partials.data_ptr(), nparts, grad_scale, max_norm, out.data_ptr(), stream()) == 0


# ---- 1. the accumulate kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_phases_are_exact_and_stay_inside_the_range(n):
    L = _lib.lib()
    gen = torch.Generator(device="cuda").manual_seed(n)
    g1, g2, g3, g4 = (_wide(n, gen) for _ in range(4))
    abuf, accum = _guarded(n)
    gbuf, grads = _guarded(n)
    run = lambda phase: L.plb_launch_grad_accum(accum.data_ptr(), grads.data_ptr(), n, phase, None, stream())
    grads.copy_(g1)
    assert run(0) == 0
    assert torch.equal(accum, g1) and torch.equal(grads, g1)
    grads.copy_(g2)
    assert run(1) == 0
    grads.copy_(g3)
    assert run(1) == 0
    assert torch.equal(accum, (g1 + g2) + g3) and torch.equal(grads, g3)
    grads.copy_(g4)
    assert run(2) == 0
    assert torch.equal(grads, ((g1 + g2) + g3) + g4)
    assert torch.equal(accum, (g1 + g2) + g3)              # LAST leaves the accumulator alone
    grads.fill_(float("nan"))                               # phase 3 never reads the gradient range
    assert run(3) == 0
    assert torch.equal(grads, accum)
    torch.cuda.synchronize()
    assert _guards_intact(abuf, n) and _guards_intact(gbuf, n)
    # what the launcher refuses: a length that is no multiple of 4, an unknown phase, partial sums before the last pass
    assert L.plb_launch_grad_accum(accum.data_ptr(), grads.data_ptr(), n + 2, 0, None, stream()) != 0
    assert L.plb_launch_grad_accum(accum.data_ptr(), grads.data_ptr(), n, 4, None, stream()) != 0
    assert L.plb_launch_grad_accum(accum.data_ptr(), grads.data_ptr(), n, 1, accum.data_ptr(), stream()) != 0


# ---- 2. the norm ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_norm_through_both_kernels_is_within_the_chain_bound_and_reproducible(n):
    L = _lib.lib()
    gen = torch.Generator(device="cuda").manual_seed(1000 + n)
    a, b = _wide(n, gen), _wide(n, gen)
    v = a + b
    scale = 0.125
    want = scale * float(v.double().pow(2).sum().sqrt())
    bound = _norm_bound(n)
    outs = []
    for rep in range(2):
        # (i) sum of squares alone
        pbuf, part = _guarded(PARTS, fill=-7.0)
        vbuf, vv = _guarded(n)
        vv.copy_(v)
        out = torch.full((4,), 9.0, device="cuda")
        assert L.plb_launch_grad_sumsq(vv.data_ptr(), n, part.data_ptr(), stream()) == 0
        _finish(L, part, PARTS, scale, 0.0, out)
        # (ii) the partials of a LAST pass that stores the same values
        p2buf, part2 = _guarded(PARTS, fill=-7.0)
        abuf, accum = _guarded(n)
        gbuf, grads = _guarded(n)
        accum.copy_(a)
        grads.copy_(b)
        out2 = torch.full((4,), 9.0, device="cuda")
        assert L.plb_launch_grad_accum(accum.data_ptr(), grads.data_ptr(), n, 2, part2.data_ptr(), stream()) == 0
        _finish(L, part2, PARTS, scale, 0.0, out2)
        torch.cuda.synchronize()
        assert torch.equal(grads, v) and torch.equal(vv, v)
        for buf, m in ((pbuf, PARTS), (p2buf, PARTS), (vbuf, n), (abuf, n), (gbuf, n)):
            assert _guards_intact(buf, m, fill=float(buf[0]))
        # workgroups whose chunk is empty write 0
        busy = -(-n // _lib.norm_chunk(n))
        assert bool((part[busy:] == 0).all()) and bool((part[:busy] >= 0).all())
        assert torch.equal(part, part2)
        assert out[:3].view(torch.int32).tolist() == out2[:3].view(torch.int32).tolist()
        assert float(out[3]) == 9.0                                   # the count of left-out updates is not the finish's
        print(f"n={n}: norm {float(out[0])!r} want {want!r} rel {abs(float(out[0]) - want) / want:.3e} bound {bound:.3e}")
        assert abs(float(out[0]) - want) <= bound * want
        assert float(out[1]) == 1.0 and float(out[2]) == 0.0         # max_norm 0: no clipping
        outs.append(out[:3].clone())
    assert outs[0].view(torch.int32).tolist() == outs[1].view(torch.int32).tolist()   # run to run: the same bits
    # the coefficient: max_norm = half the norm and ten times the norm (torch's constants: max_norm / (norm + 1e-6))
    for max_norm, expect in ((0.5 * want, 0.5 * want / (want + 1e-6)), (10.0 * want, 1.0)):
        _finish(L, part, PARTS, scale, max_norm, out)
        torch.cuda.synchronize()
        if expect == 1.0:
            assert float(out[1]) == 1.0
        else:
            print(f"n={n}: coef {float(out[1])!r} want {expect!r}")
            assert abs(float(out[1]) - expect) <= bound * expect
        assert float(out[2]) == 0.0


def _engine(num_tokens=0, seed=3):
    eng = HipEngine(_cfg(), 188, num_tokens, max_batch=4, max_seq=32)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(_cfg(), 188, num_tokens, seed=seed))
    eng._bind()
    eng.sync_weights()
    return eng


def _live_head(eng):
    """An engine on which no backward call has run steps [0, trainable), as after plb_loss_fwd_bwd."""
    return eng.trainable


@pytest.mark.parametrize("n", SIZES)
def test_plb_grad_norm_on_the_engine_range(n):
    """plb_grad_norm sums the range plb_adamw_step steps — the engine's, not the caller's: the values occupy the first
    min(n, trainable) floats of it, the rest holds exact zeros (which add nothing); the bound is the one of the range's
    length."""
    eng = _engine()
    nt = _live_head(eng)
    m = min(n, nt)
    gen = torch.Generator(device="cuda").manual_seed(2000 + n)
    eng.grads.zero_()
    eng.grads[:m].copy_(_wide(m, gen))
    eng.grads[nt:].fill_(1e3)                                          # the pooler range is not part of the norm
    want = 0.25 * float(eng.grads[:nt].double().pow(2).sum().sqrt())
    bound = _norm_bound(nt)
    nb = eng.grad_norm(0.25, 0.0)
    first = nb[:4].clone()
    nb2 = eng.grad_norm(0.25, 0.5 * want)
    torch.cuda.synchronize()
    print(f"n={n}: plb_grad_norm {float(first[0])!r} want {want!r} bound {bound:.3e}")
    assert abs(float(first[0]) - want) <= bound * want
    assert float(first[1]) == 1.0 and float(first[2]) == 0.0 and float(first[3]) == 0.0
    assert float(nb2[0]) == float(first[0])
    expect = 0.5 * want / (want + 1e-6)
    assert abs(float(nb2[1]) - expect) <= bound * expect
    assert float(eng.grad_norm(0.25, 10.0 * want)[1]) == 1.0


def test_a_non_finite_norm_leaves_the_update_out_and_counts_it():
    eng = _engine()
    nt = eng.trainable
    gen = torch.Generator(device="cuda").manual_seed(7)
    eng.grads[:nt].copy_(_wide(nt, gen))
    eng.adamw_step(1, lr=1e-3)                                         # moments that are not all zero
    eng.grads[:nt].copy_(_wide(nt, gen))
    eng.grads[12345] = float("inf")
    before = [t.clone() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.workspace)]
    nb = eng.grad_norm(1.0, 1.0)
    eng.adamw_step(2, lr=1e-3, norm_buf=nb)
    torch.cuda.synchronize()
    assert float(nb[2]) == 1.0 and float(nb[1]) == 0.0 and not np.isfinite(float(nb[0]))
    assert float(nb[3]) == 1.0
    for t, b in zip((eng.params, eng.exp_avg, eng.exp_avg_sq, eng.workspace), before):
        assert torch.equal(t, b)                                       # the workspace holds the bf16 / transposed copies
    # a finite norm afterwards: the flag clears, the count stays, the update happens
    eng.grads[12345] = 0.0
    nb = eng.grad_norm(1.0, 1.0)
    eng.adamw_step(2, lr=1e-3, norm_buf=nb)
    torch.cuda.synchronize()
    assert float(nb[2]) == 0.0 and float(nb[3]) == 1.0 and 0.0 < float(nb[1]) <= 1.0
    assert not torch.equal(eng.params[:nt], before[0][:nt])


# ---- 3. the clipped AdamW -----------------------------------------------------------------------------------------------
def test_clipped_launcher_equals_the_plain_one_at_coef_one_and_skips_on_the_flag():
    L = _lib.lib()
    n = 1024 * 3 + 4
    gen = torch.Generator(device="cuda").manual_seed(11)
    g = _wide(n, gen)
    state = lambda: [torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(s)) * sc
                     for s, sc in ((1, 0.02), (2, 1e-3))] + [torch.rand(n, device="cuda") * 0 + 1e-6]
    res = []
    for clipped in (False, True):
        p, m, v = state()
        pbuf, pb = torch.zeros(n + 16, dtype=torch.bfloat16, device="cuda"), None
        pb = pbuf[8:8 + n]
        args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), pb.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3,
                0.125, None, 0)
        if clipped:
            norm = torch.tensor([5.0, 1.0, 0.0, 0.0], device="cuda")
            assert L.plb_launch_adamw_clipped(*args, norm.data_ptr(), 1, stream()) == 0
        else:
            assert L.plb_launch_adamw(*args, stream()) == 0
        torch.cuda.synchronize()
        assert bool((pbuf[:8] == 0).all()) and bool((pbuf[8 + n:] == 0).all())
        res.append((p, m, v, pb.clone()))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert not torch.equal(res[0][0], state()[0])
    # the flag: nothing is written, the count grows (only where asked to)
    p, m, v = state()
    keep = [t.clone() for t in (p, m, v)]
    norm = torch.tensor([float("inf"), 0.0, 1.0, 2.0], device="cuda")
    args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3, 0.125, None, 0)
    assert L.plb_launch_adamw_clipped(*args, norm.data_ptr(), 1, stream()) == 0
    assert L.plb_launch_adamw_clipped(*args, norm.data_ptr(), 0, stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((p, m, v), keep)) and norm.tolist()[2:] == [1.0, 3.0]


def _five_steps(eng, mode, grad_scale, lr, clip_to=0.0, ref=None):
    """mode 'plain': plb_adamw_step; 'clipped': plb_grad_norm + plb_adamw_step_clipped with max_norm = clip_to x the step's
    own norm (these gradients' norm is set by their few largest elements and moves by orders of magnitude from step to step:
    a fixed max_norm would clip one step in five). ref = (parameter, optimizer): torch's AdamW is fed (g * grad_scale) * coef
    with coef read back from the norm buffer."""
    n = eng.trainable
    gen = torch.Generator(device="cuda").manual_seed(5)
    coefs = []
    for step in range(1, 6):
        g = _wide(n, gen)
        eng.grads[:n].copy_(g)
        if mode == "plain":
            eng.adamw_step(step, lr=lr, grad_scale=grad_scale)
            continue
        want = grad_scale * float(g.double().pow(2).sum().sqrt())
        nb = eng.grad_norm(grad_scale, clip_to * want)
        eng.adamw_step(step, lr=lr, grad_scale=grad_scale, norm_buf=nb)
        coefs.append(float(nb[1]))
        if ref is not None:
            assert abs(float(nb[0]) - want) <= _norm_bound(n) * want
            ref[0].grad = (g * grad_scale) * nb[1]
            ref[1].step()
    torch.cuda.synchronize()
    return coefs


@pytest.mark.parametrize("grad_scale,lr", [(1.0, 7e-5), (0.125, 1e-3)])
def test_clipped_adamw_against_the_plain_step_and_torch(grad_scale, lr):
    plain, unclipped, clipped = _engine(), _engine(), _engine()
    n = plain.trainable
    p0 = plain.params.clone()
    _five_steps(plain, "plain", grad_scale, lr)
    # (a) coef == 1: bit-equal to plb_adamw_step — parameters, moments, and the bf16 / transposed copies in the workspace
    coefs = _five_steps(unclipped, "clipped", grad_scale, lr, clip_to=0.0)
    assert coefs == [1.0] * 5
    for a, b, what in ((unclipped.params, plain.params, "parameters"), (unclipped.exp_avg, plain.exp_avg, "exp_avg"),
                       (unclipped.exp_avg_sq, plain.exp_avg_sq, "exp_avg_sq")):
        assert_same_bits(plain, a, b, what)
    assert torch.equal(unclipped.workspace, plain.workspace)
    # (b) clipping active, against torch.optim.AdamW on the clipped mean gradient
    p_ref = torch.nn.Parameter(p0[:n].clone())
    opt = torch.optim.AdamW([p_ref], lr=lr, weight_decay=0.01)
    coefs = _five_steps(clipped, "clipped", grad_scale, lr, clip_to=0.3, ref=(p_ref, opt))
    assert all(0.29 < c < 0.31 for c in coefs), coefs
    st = opt.state[p_ref]
    assert rel_l2(clipped.params[:n], p_ref.detach()) < 1e-6
    assert float((clipped.params[:n] - p_ref.detach()).abs().max()) < 1e-6 * float(p_ref.detach().abs().max()) + 1e-9
    assert rel_l2(clipped.exp_avg[:n], st["exp_avg"]) < 1e-6
    assert rel_l2(clipped.exp_avg_sq[:n], st["exp_avg_sq"]) < 1e-6
    assert rel_l2(clipped.params[:n] - p0[:n], p_ref.detach() - p0[:n]) < 1e-4
    # (c) clipping changed the result; (d) the pooler range never moves
    assert not torch.equal(clipped.params[:n], plain.params[:n])
    assert rel_l2(clipped.exp_avg[:n], plain.exp_avg[:n]) > 0.1
    assert torch.equal(clipped.params[n:], p0[n:]) and torch.equal(unclipped.params[n:], p0[n:])
    assert not bool(clipped.exp_avg[n:].any()) and not bool(clipped.exp_avg_sq[n:].any())


# ---- 4. ranges and liveness ------------------------------------------------------------------------------------------------
def _ragged(seed, lengths, S=32):
    """labels, masked, lengths, index lists: synthetic_batch cut to ragged lengths, every sample with a masked position."""
    labels, masked, _, idx = plbert_amd.synthetic_batch(len(lengths), S, seed=seed)
    out = []
    for b, n in enumerate(lengths):
        keep = [i for i in idx[b] if i < n] or [n // 2]
        out.append(keep)
        labels[b, n:] = 0
        masked[b, n:] = 0
    return labels, masked, np.asarray(lengths, np.int32), out


def test_window_of_a_dual_head_and_a_phoneme_only_micro_step():
    NT = 8
    sd = plbert_amd.deterministic_state_dict(_cfg(), 188, NT, seed=4)
    tr = PLBertTrainer(_cfg(), 188, max_batch=4, max_seq=32, lr=1e-3, state_dict=sd, num_tokens=NT)
    eng = tr.engine
    lab, msk, lens, idx = _ragged(21, [32, 17, 25, 9])
    tok = np.random.RandomState(5).randint(0, NT, size=lab.shape).astype(np.int64)
    dual = tr.stage_batch(lab, msk, lens, idx, token_ids=tok)
    lab2, msk2, lens2, idx2 = _ragged(22, [30, 32, 12, 21])
    mono = tr.stage_batch(lab2, msk2, lens2, idx2)
    nt, (ta, tb) = eng.trainable, eng.token_range
    tr.loss_and_grads(dual)
    g_dual = eng.grads.clone()
    eng.grad_accum_add(eng.GRAD_FIRST)
    tr.loss_and_grads(mono)
    g_mono = eng.grads.clone()
    assert torch.equal(g_mono[ta:tb], g_dual[ta:tb])              # a phoneme-only call leaves the token range alone ...
    eng.grads[ta:tb].fill_(float("nan"))                          # ... and LAST does not read it: the micro-step produced none
    pool = eng.grads[nt:ta].clone()
    eng.grad_accum_add(eng.GRAD_LAST, want_partials=True)
    torch.cuda.synchronize()
    assert torch.equal(eng.grads[ta:tb], g_dual[ta:tb])           # the dual step's token gradients, bit for bit
    assert_same_bits(eng, eng.grads[:nt], g_dual[:nt] + g_mono[:nt], "accumulated trainable range")
    assert torch.equal(eng.grads[nt:ta], pool)                    # nothing between the ranges is touched
    # the norm from the LAST pass's partials covers both ranges; the clipped update steps the token head once
    live = torch.cat([eng.grads[:nt], eng.grads[ta:tb]]).double()
    want = 0.5 * float(live.pow(2).sum().sqrt())
    nb = eng.grad_norm(0.5, 0.5 * want, have_partials=True)
    from_partials = nb[:4].clone()
    one_pass = eng.grad_norm(0.5, 0.5 * want)[:4].clone()
    assert abs(float(from_partials[0]) - want) <= _norm_bound(nt) * want
    assert abs(float(one_pass[0]) - want) <= _norm_bound(nt) * want
    steps, p0 = eng.token_head_steps, eng.params.clone()
    eng.adamw_step(1, lr=1e-3, grad_scale=0.5, norm_buf=nb)
    torch.cuda.synchronize()
    assert eng.token_head_steps == steps + 1
    assert not torch.equal(eng.params[ta:tb], p0[ta:tb]) and not torch.equal(eng.params[:nt], p0[:nt])
    assert torch.equal(eng.params[nt:ta], p0[nt:ta])
    assert eng.status()["ln_exchange_timeouts"] == 0
    # the other order: the token range joins the window at its second micro-step and starts from that copy
    tr.loss_and_grads(mono)
    eng.grad_accum_add(eng.GRAD_FIRST)
    tr.loss_and_grads(dual)
    g2 = eng.grads.clone()
    eng.grad_accum_add(eng.GRAD_ADD)
    tr.loss_and_grads(mono)
    g3 = eng.grads.clone()
    eng.grads[ta:tb].fill_(float("nan"))
    eng.grad_accum_add(eng.GRAD_LAST)
    steps = eng.token_head_steps
    eng.adamw_step(2, lr=1e-3, grad_scale=1.0 / 3)
    torch.cuda.synchronize()
    assert torch.equal(eng.grads[ta:tb], g2[ta:tb]) and eng.token_head_steps == steps + 1
    assert bool(torch.isfinite(eng.params).all())
    del g3


def test_window_of_two_encode_backwards_keeps_the_head_out_and_the_stash_alive():
    eng = _engine(seed=6)
    nt = eng.trainable
    hw = eng.layout["phoneme_predictor.weight"][0]
    rs = np.random.RandomState(3)
    ids = rs.randint(1, 180, size=(4, 32))
    lens = np.asarray([32, 20, 27, 11], np.int32)
    gen = torch.Generator(device="cuda").manual_seed(9)
    d1 = torch.randn(4, 32, 128, device="cuda", generator=gen)
    d2 = torch.randn(4, 32, 128, device="cuda", generator=gen)
    eng.encode(ids, lens)
    eng.encode_bwd(d1)
    g1 = eng.grads.clone()
    eng.encode(ids, lens)                       # the second micro-step's stash is live across the add
    eng.grad_accum_add(eng.GRAD_FIRST)
    eng.encode_bwd(d2)                          # fails ("no live stash ...") if the add had dropped it
    g2 = eng.grads.clone()
    eng.grad_accum_add(eng.GRAD_LAST, want_partials=True)
    torch.cuda.synchronize()
    assert_same_bits(eng, eng.grads[:hw], g1[:hw] + g2[:hw], "accumulated encoder range")
    assert not bool(eng.grads[hw:nt].any())      # the head range stays zeros
    p0, m0 = eng.params.clone(), eng.exp_avg.clone()
    want = 0.5 * float(eng.grads[:hw].double().pow(2).sum().sqrt())
    nb = eng.grad_norm(0.5, 0.0, have_partials=True)
    assert abs(float(nb[0]) - want) <= _norm_bound(hw) * want
    eng.adamw_step(1, lr=1e-3, grad_scale=0.5, norm_buf=nb)
    torch.cuda.synchronize()
    assert torch.equal(eng.params[hw:], p0[hw:]) and torch.equal(eng.exp_avg[hw:], m0[hw:])   # the head is not stepped
    assert not torch.equal(eng.params[:hw], p0[:hw])


def test_window_misuse_on_a_bound_engine():
    tr = PLBertTrainer(_cfg(), 188, max_batch=4, max_seq=32, lr=1e-3, seed=1)
    eng = tr.engine
    batch = tr.stage_batch(*_ragged(31, [32, 17, 25, 9]))
    tr.loss_and_grads(batch)
    eng.grad_accum_add(eng.GRAD_FIRST)
    with pytest.raises(RuntimeError, match="added twice"):
        eng.grad_accum_add(eng.GRAD_ADD)
    tr.loss_and_grads(batch)
    eng.adamw_step(1, lr=1e-3)                    # moves the parameters: the window is over
    before = eng.grads.clone()
    with pytest.raises(RuntimeError, match="plb_adamw_step moved the weights"):
        eng.grad_accum_add(eng.GRAD_LAST)
    tr.loss_and_grads(batch)
    eng.grad_accum_add(eng.GRAD_FIRST)
    tr.loss_and_grads(batch)
    eng.sync_weights()
    with pytest.raises(RuntimeError, match="plb_sync_weights"):
        eng.grad_accum_add(eng.GRAD_ADD)
    with pytest.raises(RuntimeError, match="left none in this buffer"):
        eng.grad_norm(1.0, 1.0, have_partials=True)
    torch.cuda.synchronize()
    assert before.shape == eng.grads.shape


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_step_accumulated_equals_one_step_on_the_whole_batch(packed):
    """Two bf16 evaluations of one function in another summation order (tests/test_gpu_packed.py): loss 1e-4 relative, every
    gradient tensor 1.5e-2 relative L2, and the same bound on the update p - p0."""
    sd = plbert_amd.deterministic_state_dict(_cfg(), 188, seed=8)
    lab, msk, lens, idx = _ragged(41, [32, 19, 26, 11])
    assert all(len(i) >= 1 for i in idx)
    mk = lambda: PLBertTrainer(_cfg(), 188, max_batch=4, max_seq=32, lr=1e-3, state_dict=sd, packed=packed)
    acc, one = mk(), mk()
    p0 = one.engine.params.clone()
    halves = [acc.stage_batch(lab[s], msk[s], lens[s], idx[s]) for s in (slice(0, 2), slice(2, 4))]
    loss_acc = acc.step_accumulated(halves)
    loss_one = one.step(one.stage_batch(lab, msk, lens, idx))
    torch.cuda.synchronize()
    la, lo = float(loss_acc.item()), float(loss_one.item())
    print(f"packed={packed}: mean micro-step loss {la!r}, loss of 4 {lo!r}")
    assert abs(la - lo) <= 1e-4 * lo
    assert acc.step_count == one.step_count == 1
    worst = 0.0
    for k, (o, sz, _) in one.engine.layout.items():
        if o + sz > one.engine.trainable:
            continue
        r = rel_l2(acc.engine.grads[o:o + sz] * 0.5, one.engine.grads[o:o + sz])
        worst = max(worst, r)
        assert r < 1.5e-2, (k, r)
    n = one.engine.trainable
    ru = rel_l2(acc.engine.params[:n] - p0[:n], one.engine.params[:n] - p0[:n])
    print(f"packed={packed}: worst gradient tensor {worst:.3e}, update {ru:.3e}")
    assert ru < 1.5e-2
    assert float((one.engine.params[:n] - p0[:n]).abs().max()) > 0.5e-3          # the step moved the parameters
    assert torch.equal(acc.engine.params[n:], p0[n:])
    assert acc.engine.status()["ln_exchange_timeouts"] == 0


def test_clipping_trainer_keeps_the_norm_on_the_device():
    sd = plbert_amd.deterministic_state_dict(_cfg(), 188, seed=8)
    lab, msk, lens, idx = _ragged(41, [32, 19, 26, 11])
    tr = PLBertTrainer(_cfg(), 188, max_batch=4, max_seq=32, lr=1e-3, state_dict=sd, max_grad_norm=1e-3)
    ref = PLBertTrainer(_cfg(), 188, max_batch=4, max_seq=32, lr=1e-3, state_dict=sd)
    assert ref.max_grad_norm is None and ref.last_grad_norm is None
    batch = tr.stage_batch(lab, msk, lens, idx)
    tr.step(batch)
    ref.step(ref.stage_batch(lab, msk, lens, idx))
    torch.cuda.synchronize()
    n = tr.engine.trainable
    want = float(ref.engine.grads[:n].double().pow(2).sum().sqrt())
    got = tr.last_grad_norm
    assert got.is_cuda and got.shape == (4,)
    assert abs(float(got[0]) - want) <= 1e-3 * want and 0.0 < float(got[1]) < 1.0 and float(got[2]) == 0.0
    assert abs(float(got[1]) - 1e-3 / (want + 1e-6)) <= 1e-3 * float(got[1])
    halves = [tr.stage_batch(lab[s], msk[s], lens[s], idx[s]) for s in (slice(0, 2), slice(2, 4))]
    tr.step_accumulated(halves)
    torch.cuda.synchronize()
    assert tr.step_count == 2 and float(tr.last_grad_norm[2]) == 0.0 and float(tr.last_grad_norm[0]) > 0.0


# ---- 6. the default step launches what it launched ------------------------------------------------------------------------
def test_default_step_launches_are_unchanged_by_the_new_entry_points():
    sd = plbert_amd.deterministic_state_dict(_cfg(), 188, seed=8)
    lab, msk, lens, idx = _ragged(41, [32, 19, 26, 11])

    def counts(tr):
        batch = tr.stage_batch(lab, msk, lens, idx)
        tr.step(batch)                               # warm: weight copies are in place, nothing left to sync
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        try:
            _lib.profile_read()
            tr.step(batch)
            torch.cuda.synchronize()
            return {k: v["launches"] for k, v in _lib.profile_read().items()}
        finally:
            _lib.profile_enable(False)

    mk = lambda: PLBertTrainer(_cfg(), 188, max_batch=4, max_seq=32, lr=1e-3, state_dict=sd)
    fresh = mk()
    base = counts(fresh)
    used = mk()
    if hasattr(used, "step_accumulated"):            # every new entry point once, then the default step again
        halves = [used.stage_batch(lab[s], msk[s], lens[s], idx[s]) for s in (slice(0, 2), slice(2, 4))]
        used.step_accumulated(halves)
        used.engine.adamw_step(used.step_count, lr=1e-3, norm_buf=used.engine.grad_norm(1.0, 1.0))
    after = counts(used)
    assert after == base, (base, after)
    assert base.get("adamw") == 1 and sum(base.values()) > 20
