"""AdamW parameter groups and frozen tensors on the GPU (-m gpu): the segmented kernels through their launchers (segment
edges, holes, guards, the clipped form, the skip word and the non-finite flag as plain input words, refusals), the masked
sum of squares, plb_adamw_step_groups against plb_adamw_step[_clipped] (one group: bit for bit) and against
torch.optim.AdamW with three groups and a frozen tensor, plbert_amd.train.AdamW built from dicts, and the unchanged default
step. Engine of tests/test_gpu_adamw_kernel.py: embedding 64, hidden 128, 2 heads, FFN 256, 2 layers, max_batch 2, max_seq 32.

Bounds. Launcher level: bit equality with one plb_launch_adamw / plb_launch_adamw_clipped call per segment, and every live
element inside the allowances of gpu_util.adamw_fp64. Against torch: the 1e-6 relative bound of
tests/test_gpu_adamw_kernel.py, per tensor. The masked norm: bit equality with the unmasked kernels on zero-filled input."""
import numpy as np
import pytest
import torch

import gpu_util as gu
from gpu_util import rel_l2, stream
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import HipEngine
from plbert_amd.train import AdamW, PLBertTrainer

pytestmark = pytest.mark.gpu

NPARAM = _lib.PLB_NPARAM
PAD = 64                                    # sentinel floats on either side of a range (the range stays 16-byte aligned)
SENT_F32, SENT_BF16 = 0x7FC0ABCD, 0x7FC1    # NaN patterns no update produces
# (begin, end) in floats. 4: a boundary inside the first wave; 1024: on a workgroup edge; 2044 / 2056: just before and just
# after one (a 12-float segment across the edge); [2056, 2064): a hole; the last segment ends at n = 4 x 1024 + 16.
# Lengths 4, 1020, 1020, 12, (8), 1028, 1020.
BOUNDS = ((0, 4), (4, 1024), (1024, 2044), (2044, 2056), (2064, 3092), (3092, 4112))
N = 4112
HYPER = ((0.9, 0.999, 1e-8), (0.8, 0.99, 1e-6), (0.95, 0.98, 1e-8))
GS = 0.125


def _cfg():
    return plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)


def _settings():
    """One (lr, wd, b1, b2, eps, step) per segment of BOUNDS, from the project's triples and step counts."""
    out = []
    for k in range(len(BOUNDS)):
        lr, wd, _ = gu.ADAMW_TRIPLES[k % len(gu.ADAMW_TRIPLES)]
        out.append((lr, wd, *HYPER[(k // 2) % len(HYPER)], gu.ADAMW_STEPS[k % len(gu.ADAMW_STEPS)]))
    return out


def _segment(begin, end, lr, wd, b1, b2, eps, step, group=0):
    """plb_adamw_plan's scalars: double expressions rounded to fp32 once (tests/test_adamw_groups_host.py holds the plan to
    the same expressions)."""
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    f = lambda x: float(np.float32(x))
    return _lib.PlbAdamWSegment(begin, end, group, step, f(1.0 - lr * wd), f(1.0 - b1), f(b2), f(1.0 - b2), f(eps), f(lr / bc1),
                                f(np.sqrt(bc2)))


def _segs(bounds=BOUNDS, settings=None):
    settings = settings or _settings()
    arr = (_lib.PlbAdamWSegment * max(1, len(bounds)))()
    for k, ((a, b), s) in enumerate(zip(bounds, settings)):
        arr[k] = _segment(a, b, *s)
    return arr


class Buffers:
    """p, g, m, v (fp32 bit patterns) and the bf16 copy of N floats, each between sentinels."""

    def __init__(self, state):
        self.t = {}
        for name, a in zip("pgmv", state):
            buf = torch.full((PAD + N + PAD,), SENT_F32, dtype=torch.int32, device="cuda")
            buf[PAD:PAD + N] = torch.from_numpy(a.view(np.int32).copy()).cuda()
            self.t[name] = buf
        self.t["b"] = torch.full((PAD + N + PAD,), SENT_BF16, dtype=torch.int16, device="cuda")

    def ptr(self, name, off=0):
        buf = self.t[name]
        return buf.data_ptr() + (PAD + off) * buf.element_size()

    def ptrs(self, off=0):
        return tuple(self.ptr(k, off) for k in "pgmvb")

    def f32(self, name):
        return self.t[name][PAD:PAD + N].cpu().numpy().view(np.float32)

    def same_bits(self, other, what):
        for k in "pgmvb":
            assert torch.equal(self.t[k], other.t[k]), f"{what}: {k} differs (guards and holes included)"


def _segmented(L, bufs, segs, nseg, skip=None, count_skip=0, norm=None, count_nonfinite=0, n=N):
    rc = L.plb_launch_adamw_segments(*bufs.ptrs(), n, segs, nseg, GS, skip.data_ptr() if skip is not None else None, count_skip,
                                     norm.data_ptr() if norm is not None else None, count_nonfinite, stream())
    torch.cuda.synchronize()
    return rc


def _per_segment(L, bufs, norm=None):
    """The reference: one plb_launch_adamw (norm: plb_launch_adamw_clipped) call per segment."""
    for (a, b), (lr, wd, b1, b2, eps, step) in zip(BOUNDS, _settings()):
        args = (*bufs.ptrs(a), b - a, lr, b1, b2, eps, wd, step, GS, None, 0)
        if norm is None:
            assert L.plb_launch_adamw(*args, stream()) == 0
        else:
            assert L.plb_launch_adamw_clipped(*args, norm.data_ptr(), 0, stream()) == 0
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def state():
    return gu.adamw_state(N)


# ---- 1. the segmented launch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coef", [None, 1.0, 0.37])
def test_segments_equal_one_launch_per_segment_bit_for_bit(state, coef):
    L = _lib.lib()
    got, want = Buffers(state), Buffers(state)
    norm = None if coef is None else torch.tensor([5.0, coef, 0.0, 2.0], dtype=torch.float32, device="cuda")
    assert _segmented(L, got, _segs(), len(BOUNDS), norm=norm, count_nonfinite=1) == 0
    _per_segment(L, want, norm)
    got.same_bits(want, f"coef={coef}")
    if norm is not None:
        assert norm.tolist() == [5.0, float(np.float32(coef)), 0.0, 2.0]        # a finite norm: nothing is counted
    # holes, guards and the gradient are bit-unchanged; the live elements moved
    fresh = Buffers(state)
    live = np.zeros(N, dtype=bool)
    for a, b in BOUNDS:
        live[a:b] = True
    for k in "pmvb":
        changed = (got.t[k] != fresh.t[k]).cpu().numpy()
        assert not changed[:PAD].any() and not changed[PAD + N:].any(), f"{k}: a guard was written"
        assert not changed[PAD:PAD + N][~live].any(), f"{k}: the hole was written"
        assert changed[PAD:PAD + N][live].mean() > 0.5, k
    assert torch.equal(got.t["g"], fresh.t["g"])
    # every live element against one step in float64 with the segment's own hyper-parameters
    p, m, v = got.f32("p"), got.f32("m"), got.f32("v")
    for (a, b), (lr, wd, b1, b2, eps, step) in zip(BOUNDS, _settings()):
        ref = gu.adamw_fp64(*(x[a:b] for x in state), lr, wd, GS, step, coef=None if coef is None else np.float32(coef),
                            b1=b1, b2=b2, eps=eps)
        gu.check_adamw(f"segment [{a}, {b}) coef={coef}", p[a:b], m[a:b], v[a:b], ref)
    gu.check_bf16_copy("bf16 copy of the live elements", got.t["b"][PAD:PAD + N].cpu().numpy().view(np.uint16)[live], p[live])


def test_one_segment_over_the_range_is_the_plain_launch(state):
    """[0, n): plb_launch_adamw's bits; with a norm buffer plb_launch_adamw_clipped's."""
    L = _lib.lib()
    lr, wd, gs = gu.ADAMW_TRIPLES[0]
    for norm_vals in (None, [3.0, 0.61, 0.0, 0.0]):
        got, want = Buffers(state), Buffers(state)
        norm = None if norm_vals is None else torch.tensor(norm_vals, dtype=torch.float32, device="cuda")
        segs = _segs(((0, N),), [(lr, wd, gu.ADAMW_B1, gu.ADAMW_B2, gu.ADAMW_EPS, 10)])
        assert _segmented(L, got, segs, 1, norm=norm) == 0
        args = (*want.ptrs(), N, lr, gu.ADAMW_B1, gu.ADAMW_B2, gu.ADAMW_EPS, wd, 10, GS, None, 0)
        if norm is None:
            assert L.plb_launch_adamw(*args, stream()) == 0
        else:
            assert L.plb_launch_adamw_clipped(*args, norm.data_ptr(), 0, stream()) == 0
        torch.cuda.synchronize()
        got.same_bits(want, f"one segment, norm={norm_vals}")


@pytest.mark.parametrize("clipped", [False, True])
def test_skip_word_and_nonfinite_flag_write_nothing_and_count_once(state, clipped):
    L = _lib.lib()
    bufs, fresh = Buffers(state), Buffers(state)
    norm = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float32, device="cuda") if clipped else None
    for count_skip in (0, 1, 2):
        skip = torch.tensor([3, 10, 20, 30], dtype=torch.int32, device="cuda")     # a caller-owned word
        for k in range(2):
            assert _segmented(L, bufs, _segs(), len(BOUNDS), skip=skip, count_skip=count_skip, norm=norm, count_nonfinite=1) == 0
            want = [3, 10, 20, 30]
            if count_skip:
                want[count_skip] += k + 1                                            # one per launch (five workgroups ran)
            assert skip.tolist() == want
    bufs.same_bits(fresh, "skip[0] != 0")
    if clipped:
        assert norm.tolist() == [1.0, 1.0, 0.0, 0.0]                                # the skip word is tested first
        bad = torch.tensor([float("inf"), 0.0, 1.0, 2.0], dtype=torch.float32, device="cuda")
        skip = torch.tensor([0, 10, 20, 30], dtype=torch.int32, device="cuda")
        assert _segmented(L, bufs, _segs(), len(BOUNDS), skip=skip, count_skip=1, norm=bad, count_nonfinite=1) == 0
        assert bad.tolist()[2:] == [1.0, 3.0]
        assert _segmented(L, bufs, _segs(), len(BOUNDS), skip=skip, count_skip=1, norm=bad, count_nonfinite=0) == 0
        assert bad.tolist()[2:] == [1.0, 3.0] and skip.tolist() == [0, 10, 20, 30]
        bufs.same_bits(fresh, "norm[2] != 0")


def test_launcher_refusals_write_nothing(state):
    L = _lib.lib()
    bufs, fresh = Buffers(state), Buffers(state)
    s = _settings()
    bad = [((0, 6), (8, 16)),                      # a boundary that is no multiple of 4
           ((0, 8), (4, 16)),                      # overlapping
           ((8, 16), (0, 8)),                      # unsorted
           ((0, 8), (8, 8)),                       # empty
           ((0, 8), (8, N + 4))]                   # beyond n
    for bounds in bad:
        assert _segmented(L, bufs, _segs(bounds, s), len(bounds)) != 0, bounds
    many = tuple((8 * k, 8 * k + 4) for k in range(NPARAM + 1))
    arr = (_lib.PlbAdamWSegment * (NPARAM + 1))(*[_segment(a, b, *s[0]) for a, b in many])
    assert _segmented(L, bufs, arr, NPARAM + 1) != 0                               # more than PLB_NPARAM segments
    for step in (0, -1):
        one = _segs(((0, 8),), s)
        one[0].step = step                                                          # (the scalars of a valid step)
        assert _segmented(L, bufs, one, 1) != 0
    assert _segmented(L, bufs, _segs(), len(BOUNDS), n=N + 2) != 0                 # n itself
    part = torch.zeros(_lib.PLB_NORM_PARTS, device="cuda")
    for bounds in bad:
        assert L.plb_launch_grad_sumsq_segments(bufs.ptr("g"), N, _segs(bounds, s), len(bounds), part.data_ptr(), stream()) != 0
    assert _segmented(L, Buffers(state), _segs(), 0) == 0                          # no segment: nothing is launched
    torch.cuda.synchronize()
    bufs.same_bits(fresh, "refused")
    # PLB_NPARAM four-float segments are accepted, and only they are written
    got = Buffers(state)
    assert _segmented(L, got, arr, NPARAM) == 0
    changed = (got.t["p"] != fresh.t["p"]).cpu().numpy()[PAD:PAD + N]
    inside = np.zeros(N, dtype=bool)
    for a, b in many[:NPARAM]:
        inside[a:b] = True
    assert not changed[~inside].any() and changed[inside].any()


# ---- 2. the masked sum of squares ----------------------------------------------------------------------------------------
# 4112: BOUNDS; the large one: a chunk of two passes per workgroup, holes inside a pass, across passes and across workgroups
BIG = _lib.PLB_NORM_PARTS * 1024 + 4
BIG_BOUNDS = ((0, 4), (4, 1020), (1028, 2044), (2056, 5000), (6148, 300000), (300004, BIG - 8), (BIG - 4, BIG))


@pytest.mark.parametrize("n,bounds", [(N, BOUNDS), (BIG, BIG_BOUNDS)])
def test_masked_sumsq_equals_the_plain_one_on_a_zero_filled_copy(n, bounds):
    L = _lib.lib()
    gen = torch.Generator(device="cuda").manual_seed(n)
    g = torch.randn(n, device="cuda", generator=gen) * torch.exp(torch.randn(n, device="cuda", generator=gen) * 3 - 6)
    live = torch.zeros(n, dtype=torch.bool, device="cuda")
    for a, b in bounds:
        live[a:b] = True
    zeroed = torch.where(live, g, torch.zeros_like(g))
    poisoned = g.clone()
    holes = (~live).nonzero().flatten()
    assert holes.numel() >= 8
    poisoned[holes[0::3]] = float("nan")
    poisoned[holes[1::3]] = float("inf")
    poisoned[holes[2::3]] = -1e30
    settings = [_settings()[0]] * len(bounds)
    want = torch.full((_lib.PLB_NORM_PARTS,), -7.0, device="cuda")
    assert L.plb_launch_grad_sumsq(zeroed.data_ptr(), n, want.data_ptr(), stream()) == 0
    for src in (g, poisoned):
        keep = src.clone()
        got = torch.full((_lib.PLB_NORM_PARTS,), -7.0, device="cuda")
        assert L.plb_launch_grad_sumsq_segments(src.data_ptr(), n, _segs(bounds, settings), len(bounds), got.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.equal(src.view(torch.int32), keep.view(torch.int32))           # the gradients are only read
    assert bool(torch.isfinite(want).all()) and float(want.sum()) > 0
    # one segment over everything is the plain kernel; no segment at all gives zeros
    full = torch.empty_like(want)
    assert L.plb_launch_grad_sumsq(g.data_ptr(), n, full.data_ptr(), stream()) == 0
    one = torch.empty_like(want)
    assert L.plb_launch_grad_sumsq_segments(g.data_ptr(), n, _segs(((0, n),), settings), 1, one.data_ptr(), stream()) == 0
    none = torch.full_like(want, 3.0)
    assert L.plb_launch_grad_sumsq_segments(poisoned.data_ptr(), n, _segs((), []), 0, none.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(one.view(torch.int32), full.view(torch.int32)) and not bool(none.any())


def _engine(num_tokens=0, seed=3):
    eng = HipEngine(_cfg(), 188, num_tokens, max_batch=2, max_seq=32)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(_cfg(), 188, num_tokens, seed=seed))
    eng._bind()
    eng.sync_weights()
    return eng


def _wide(n, gen):
    g = torch.randn(n, device="cuda", generator=gen) * torch.exp(torch.randn(n, device="cuda", generator=gen) * 3 - 6)
    g[::97] = 0.0
    return g


FROZEN = ("encoder.embeddings.position_embeddings.weight", "encoder.encoder.albert_layer_groups.0.albert_layers.0.ffn.bias",
          "encoder.embeddings.LayerNorm.weight")


def test_plb_grad_norm_groups_is_plb_grad_norm_on_zeroed_frozen_gradients():
    eng = _engine()
    nt = eng.trainable
    eng.grads[:nt].copy_(_wide(nt, torch.Generator(device="cuda").manual_seed(77)))
    eng.grads[nt:].fill_(1e3)                                                      # the pooler is no part of either norm
    group_of = {n: 0 for n in eng.layout if n not in FROZEN}
    for n in FROZEN:
        off, size, _ = eng.layout[n]
        eng.grads[off:off + size:5] = float("nan")
    got = eng.grad_norm(0.25, 0.01, group_of=group_of)[:4].clone()
    for n in FROZEN:
        off, size, _ = eng.layout[n]
        eng.grads[off:off + size].zero_()
    want = eng.grad_norm(0.25, 0.01)[:4].clone()
    torch.cuda.synchronize()
    assert torch.equal(got[:3].view(torch.int32), want[:3].view(torch.int32)), (got.tolist(), want.tolist())
    assert float(got[2]) == 0.0 and 0.0 < float(got[1]) < 1.0 and float(got[0]) > 0.0
    with pytest.raises(RuntimeError, match="group_of"):
        eng.grad_norm(1.0, 0.0, group_of=[0] * (NPARAM - 1) + [-2])


# ---- 3. one group is the old step -----------------------------------------------------------------------------------------
def _ragged2(seed):
    labels, masked, _, idx = plbert_amd.synthetic_batch(2, 32, seed=seed)
    lens = [32, 19]
    out = []
    for b, n in enumerate(lens):
        out.append([i for i in idx[b] if i < n] or [n // 2])
        labels[b, n:] = 0
        masked[b, n:] = 0
    return labels, masked, np.asarray(lens, np.int32), out


@pytest.mark.parametrize("mode", ["plain", "clipped", "dual", "encode_bwd"])
def test_one_group_for_every_tensor_is_the_old_step(mode):
    NT = 8 if mode == "dual" else 0
    sd = plbert_amd.deterministic_state_dict(_cfg(), 188, NT, seed=4)
    mk = lambda: PLBertTrainer(_cfg(), 188, max_batch=2, max_seq=32, lr=1e-3, state_dict=sd, num_tokens=NT)
    old, new = mk(), mk()
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    lab, msk, lens, idx = _ragged2(21)
    tok = np.random.RandomState(5).randint(0, max(NT, 1), size=lab.shape).astype(np.int64) if NT else None
    ids = np.random.RandomState(3).randint(1, 180, size=(2, 32))
    d = torch.randn(2, 32, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    for step in (1, 2, 3):
        for tr in (old, new):
            if mode == "encode_bwd":
                tr.engine.encode(ids, lens)
                tr.engine.encode_bwd(d)
            else:
                tr.loss_and_grads(tr.stage_batch(lab, msk, lens, idx, token_ids=tok))
        new.engine.grads.copy_(old.engine.grads)                                    # the same gradient bits, whatever made them
        if mode == "dual" and step == 1:                                           # the token head's own count in the plan
            plan = new.engine.adamw_plan(5, [hyper], [0] * NPARAM)
            ta, tb = new.engine.token_range
            assert [(s["begin"], s["end"], s["step"]) for s in plan] == [(0, new.engine.trainable, 5), (ta, tb, 1)]
        if mode == "encode_bwd" and step == 1:                                      # the head has no gradient: not in the plan
            plan = new.engine.adamw_plan(5, [hyper], [0] * NPARAM)
            assert [(s["begin"], s["end"]) for s in plan] == [(0, new.engine.layout["phoneme_predictor.weight"][0])]
        if mode == "clipped":
            nb_old = old.engine.grad_norm(1.0, 1e-3)
            nb_new = new.engine.grad_norm(1.0, 1e-3, group_of=[0] * NPARAM)
            assert torch.equal(nb_old[:3].view(torch.int32), nb_new[:3].view(torch.int32)) and 0 < float(nb_new[1]) < 1
            old.engine.adamw_step(step, **hyper, norm_buf=nb_old)
            new.engine.adamw_step_groups(step, [hyper], [0] * NPARAM, norm_buf=nb_new)
        else:
            old.engine.adamw_step(step, **hyper)
            new.engine.adamw_step_groups(step, [hyper], [0] * NPARAM)
        torch.cuda.synchronize()
        for what in ("params", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(old.engine, what), getattr(new.engine, what)), (mode, step, what)
        assert old.engine.token_head_steps == new.engine.token_head_steps == (step if mode == "dual" else 0)
    # the compute copies, through a forward
    out_old, out_new = old.engine.forward(ids, lens), new.engine.forward(ids, lens)
    torch.cuda.synchronize()
    for a, b in zip(out_old, out_new):
        assert (a is None and b is None) or torch.equal(a, b)
    assert not torch.equal(new.engine.params[:100], torch.zeros(100, device="cuda"))
    assert new.engine.status()["ln_exchange_timeouts"] == 0


# ---- 4. groups against torch ----------------------------------------------------------------------------------------------
def _three_groups(name):
    """0: decay 0.01, lr 1e-3 | 1: biases and LayerNorm, no decay | 2: embeddings, lr 1e-4, betas (0.8, 0.99), eps 1e-6;
    the position table is frozen (-1)."""
    if "position_embeddings" in name:
        return -1
    if "embeddings." in name:
        return 2
    return 1 if ("bias" in name or "LayerNorm" in name or "layer_norm" in name) else 0


THREE = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
         dict(lr=1e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)]


def _bf16_copy(eng):
    """The flat bf16 compute copy: the first `total` 2-byte words of the workspace (csrc/engine.cpp: o_wbf is carved first).
    Checked here against the rounding of the parameters a sync has just cast."""
    wb = eng.workspace[:2 * eng.total].view(torch.int16)
    want = torch.from_numpy(gu.bf16_rne_bits(eng.params.cpu().numpy()).view(np.int16)).cuda()
    assert torch.equal(wb, want), "the flat bf16 copy is not where this test looks for it"
    return wb


def test_three_groups_and_a_frozen_tensor_against_torch():
    eng = _engine()
    n = eng.trainable
    wb = _bf16_copy(eng)
    names = [k for k, (off, size, _) in eng.layout.items() if off + size <= n]
    group_of = {k: _three_groups(k) for k in eng.layout}                           # the pooler is given a group: it stays out
    ref = {k: torch.nn.Parameter(eng.view(k).detach().clone()) for k in names}
    frozen = "encoder.embeddings.position_embeddings.weight"
    opt = torch.optim.AdamW([{"params": [ref[k] for k in names if group_of[k] == i], **THREE[i]} for i in range(3)])
    foff, fsize, _ = eng.layout[frozen]
    # sentinels in everything of the frozen tensor that a store would change
    eng.exp_avg[foff:foff + fsize].fill_(123.25)
    eng.exp_avg_sq[foff:foff + fsize].fill_(321.5)
    wb[foff:foff + fsize] = SENT_BF16
    p0, wb0 = eng.params.clone(), wb.clone()
    gen = torch.Generator(device="cuda").manual_seed(5)
    for step in range(1, 6):
        g = _wide(n, gen)
        eng.grads[:n].copy_(g)
        eng.grads[foff:foff + fsize:7] = float("nan")                              # never read
        for k in names:
            off, size, shp = eng.layout[k]
            ref[k].grad = g[off:off + size].view(shp).clone()
        opt.step()
        eng.adamw_step_groups(step, THREE, group_of)
    torch.cuda.synchronize()
    moved = {0: 0.0, 1: 0.0, 2: 0.0}
    for k in names:
        off, size, shp = eng.layout[k]
        sl = slice(off, off + size)
        if k == frozen:
            continue
        st = opt.state[ref[k]]
        want = ref[k].detach().flatten()
        assert rel_l2(eng.params[sl], want) < 1e-6, k
        assert float((eng.params[sl] - want).abs().max()) < 1e-6 * float(want.abs().max()) + 1e-9, k
        assert rel_l2(eng.exp_avg[sl], st["exp_avg"].flatten()) < 1e-6, k
        assert rel_l2(eng.exp_avg_sq[sl], st["exp_avg_sq"].flatten()) < 1e-6, k
        moved[group_of[k]] = max(moved[group_of[k]], float((eng.params[sl] - p0[sl]).abs().max()))
        got_b = wb[sl].cpu().numpy().view(np.uint16)
        assert np.array_equal(got_b, gu.bf16_rne_bits(eng.params[sl].cpu().numpy())), k
    for i in range(3):                                                              # each group moved by about its own lr
        assert moved[i] > 2 * THREE[i]["lr"], (i, moved)
    assert moved[2] < 0.5 * moved[0]
    # the frozen tensor and the pooler: parameters, both moments and the bf16 copy bit-unchanged
    fs = slice(foff, foff + fsize)
    assert torch.equal(eng.params[fs], p0[fs]) and torch.equal(wb[fs], wb0[fs])
    assert bool((eng.exp_avg[fs] == 123.25).all()) and bool((eng.exp_avg_sq[fs] == 321.5).all())
    assert torch.equal(eng.params[n:], p0[n:]) and torch.equal(wb[n:], wb0[n:])
    assert not bool(eng.exp_avg[n:].any()) and not bool(eng.exp_avg_sq[n:].any())


# ---- 5. plbert_amd.train.AdamW built from dicts ---------------------------------------------------------------------------
def _model():
    cfg = _cfg()
    enc = plbert_amd.AlbertModel(cfg, max_batch=2, max_seq=32)
    return plbert_amd.PhonemeOnlyModel(enc, 188, cfg.hidden_size)


def _set_grads(model, refs, gen):
    for (n, p), r in zip(model.named_parameters(), refs):
        if "pooler" in n:
            continue
        g = torch.randn(p.shape, device="cuda", generator=gen) * 1e-2
        p.grad, r.grad = g, g.clone()


def test_python_optimizer_with_dict_groups_against_torch():
    model = _model()
    named = list(model.named_parameters())
    refs = [torch.nn.Parameter(p.detach().clone()) for _, p in named]
    pick = lambda ps, cond: [p for (n, _), p in zip(named, ps) if cond(n)]
    is_nd = lambda n: "pooler" not in n and "position" not in n and ("bias" in n or "LayerNorm" in n)
    is_d = lambda n: "pooler" not in n and "position" not in n and not is_nd(n)
    mk = lambda ps: [{"params": pick(ps, is_d), "weight_decay": 0.01}, {"params": pick(ps, is_nd), "weight_decay": 0.0, "lr": 5e-4}]
    opt = AdamW(mk([p for _, p in named]), lr=1e-3, model=model)
    tor = torch.optim.AdamW(mk(refs), lr=1e-3)
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 5e-4] and opt.param_groups[1]["betas"] == (0.9, 0.999)
    with pytest.raises(ValueError, match="some parameters appear in more than one parameter group"):
        opt.add_param_group({"params": [named[0][1]]})
    with pytest.raises(ValueError, match="not one of the model's"):
        AdamW([{"params": [torch.nn.Parameter(torch.zeros(4, device="cuda"))]}], model=model)
    pos = next(i for i, (n, _) in enumerate(named) if "position" in n)
    p_pos0 = named[pos][1].detach().clone()
    gen = torch.Generator(device="cuda").manual_seed(12)

    def both_step():
        _set_grads(model, refs, gen)
        opt.step()
        tor.step()

    def agree(what):
        torch.cuda.synchronize()
        for (n, p), r in zip(named, refs):
            assert rel_l2(p.detach(), r.detach()) < 1e-6, (what, n)

    both_step()
    both_step()
    agree("two steps")
    assert torch.equal(named[pos][1].detach(), p_pos0)                              # in no group: frozen
    sd = opt.state_dict()
    assert pos not in sd["state"] and len(sd["param_groups"]) == 2                  # never stepped: no state, as in torch
    assert all(i in sd["state"] for g in sd["param_groups"] for i in g["params"])
    assert float(sd["state"][sd["param_groups"][0]["params"][0]]["step"]) == 2.0
    # a changed lr takes effect at the next step
    for g_mine, g_tor in zip(opt.param_groups, tor.param_groups):
        g_mine["lr"] = g_tor["lr"] = 2e-3
    both_step()
    agree("after the lr change")
    # requires_grad = False and .grad = None freeze for as long as they hold
    w = next(i for i, (n, _) in enumerate(named) if n.endswith("ffn.weight"))
    named[w][1].requires_grad_(False)
    refs[w].requires_grad_(False)
    before = named[w][1].detach().clone()
    _set_grads(model, refs, gen)
    refs[w].grad = None
    b = next(i for i, (n, _) in enumerate(named) if n.endswith("ffn.bias"))
    named[b][1].grad = None
    refs[b].grad = None
    opt.step()
    tor.step()
    agree("with a frozen weight and a missing gradient")
    assert torch.equal(named[w][1].detach(), before)
    named[w][1].requires_grad_(True)
    refs[w].requires_grad_(True)
    # state_dict -> torch -> state_dict: moments and groups survive. (The shared step count: every stepped tensor reports
    # the optimizer's count, 4, where torch counted 3 for the two tensors that sat one step out.)
    sd = opt.state_dict()
    tor2 = torch.optim.AdamW(mk(refs), lr=9.0)
    tor2.load_state_dict(sd)
    assert [g["lr"] for g in tor2.param_groups] == [2e-3, 2e-3] and tor2.param_groups[1]["weight_decay"] == 0.0
    k0 = mk(refs)[0]["params"][0]
    i0 = sd["param_groups"][0]["params"][0]
    assert torch.equal(tor2.state[k0]["exp_avg"], sd["state"][i0]["exp_avg"])
    back = tor2.state_dict()
    m0, v0 = model.engine.exp_avg.clone(), model.engine.exp_avg_sq.clone()
    opt2 = AdamW(mk([p for _, p in named]), lr=9.0, model=model)
    opt2.load_state_dict(back)
    torch.cuda.synchronize()
    assert opt2.step_count == 4 and [g["lr"] for g in opt2.param_groups] == [2e-3, 2e-3]
    assert torch.equal(model.engine.exp_avg, m0) and torch.equal(model.engine.exp_avg_sq, v0)
    assert set(opt2.state_dict()["state"]) == set(sd["state"])
    with pytest.raises(ValueError, match="sizes"):
        AdamW([{"params": [p for _, p in named]}], model=model).load_state_dict(back)
    # add_param_group thaws the position table
    opt.add_param_group({"params": [named[pos][1]], "weight_decay": 0.0})
    tor.add_param_group({"params": [refs[pos]], "weight_decay": 0.0})
    p_before = named[pos][1].detach().clone()
    _set_grads(model, refs, gen)
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(named[pos][1].detach(), p_before)
    assert pos in opt.state_dict()["state"] and len(opt.param_groups) == 3
    # a genuine torch state dict: refused, before anything is written, when its per-parameter counts differ (torch counted
    # 3 for the two tensors that sat a step out and 4 for the rest; the fused update keeps ONE count) ...
    m0, v0, count = model.engine.exp_avg.clone(), model.engine.exp_avg_sq.clone(), opt.step_count
    with pytest.raises(ValueError, match="step counts differ"):
        opt.load_state_dict(tor.state_dict())
    torch.cuda.synchronize()
    assert torch.equal(model.engine.exp_avg, m0) and torch.equal(model.engine.exp_avg_sq, v0) and opt.step_count == count
    assert [g["lr"] for g in opt.param_groups][:2] == [2e-3, 2e-3]
    # ... and taken when its stepped tensors share one count
    tor3 = torch.optim.AdamW(mk(refs) + [{"params": [refs[pos]], "weight_decay": 0.0}], lr=3e-3)
    _set_grads(model, refs, gen)
    tor3.step()
    tor3.step()
    opt.load_state_dict(tor3.state_dict())
    torch.cuda.synchronize()
    assert opt.step_count == 2 and [g["lr"] for g in opt.param_groups] == [3e-3, 5e-4, 3e-3]
    off, size, shp = model.engine.layout["encoder.embeddings.position_embeddings.weight"]
    assert torch.equal(model.engine.exp_avg[off:off + size].view(shp), tor3.state[refs[pos]]["exp_avg"])
    assert set(opt.state_dict()["state"]) == {i for i, (n, _) in enumerate(named) if "pooler" not in n}


def test_a_left_out_update_does_not_count_as_a_step_of_its_tensors():
    """What the HandoffTimeout path does to the owners of a step count, with the callback called directly (no fault is
    provoked): the count goes back, and a tensor whose FIRST update was the one left out has no optimizer state."""
    class Left:
        skipped_updates = 1

    sd = plbert_amd.deterministic_state_dict(_cfg(), 188, seed=8)
    lab, msk, lens, idx = _ragged2(41)
    tr = PLBertTrainer(_cfg(), 188, max_batch=2, max_seq=32, lr=1e-3, state_dict=sd, frozen=("position_embeddings",))
    batch = tr.stage_batch(lab, msk, lens, idx)
    tr.step(batch)
    first = tr.stepped
    assert first and "encoder.embeddings.position_embeddings.weight" not in first
    tr.param_groups[0]["names"].append("encoder.embeddings.position_embeddings.weight")     # thawed for the second step
    tr.step(batch)
    assert tr.stepped == first | {"encoder.embeddings.position_embeddings.weight"} and tr.step_count == 2
    for cb in tr.engine._on_handoff_timeout:
        cb(Left())
    assert tr.step_count == 1 and tr.stepped == first
    tr.step(batch)                                                                          # and it is noted again when it does step
    assert tr.step_count == 2 and "encoder.embeddings.position_embeddings.weight" in tr.stepped
    for cb in tr.engine._on_handoff_timeout:
        cb(Left())
        cb(Left())
    assert tr.step_count == 0 and tr.stepped == set()


def test_python_optimizer_clips_with_the_masked_norm():
    model = _model()
    named = list(model.named_parameters())
    frozen = next(p for n, p in named if "word_embeddings" in n)
    frozen.requires_grad_(False)
    opt = AdamW([{"params": [p for n, p in named if "pooler" not in n]}], lr=1e-3, model=model, max_grad_norm=1e-3)
    gen = torch.Generator(device="cuda").manual_seed(13)
    total = 0.0
    for n, p in named:
        if "pooler" in n:
            continue
        p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-2
        if p is frozen:
            p.grad[0, 0] = float("nan")
        else:
            total += float(p.grad.double().pow(2).sum())
    before = frozen.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    want = total ** 0.5
    got = opt.last_grad_norm
    bound = 0.5 * (_lib.norm_chain(model.engine.trainable) + 2) * 2.0 ** -24       # tests/test_gpu_grad_accum.py
    assert abs(float(got[0]) - want) <= bound * want and float(got[2]) == 0.0
    assert abs(float(got[1]) - 1e-3 / (want + 1e-6)) <= 1e-5 * float(got[1]) and float(got[3]) == 0.0
    assert torch.equal(frozen.detach(), before) and bool(torch.isfinite(model.engine.params).all())


# ---- 6. the trainer: groups by name, and the unchanged default ------------------------------------------------------------
def test_trainer_with_no_decay_and_frozen_names():
    sd = plbert_amd.deterministic_state_dict(_cfg(), 188, seed=8)
    lab, msk, lens, idx = _ragged2(41)
    tr = PLBertTrainer(_cfg(), 188, max_batch=2, max_seq=32, lr=1e-3, state_dict=sd, no_decay=("bias", "LayerNorm"),
                       frozen=("embeddings.",), max_grad_norm=1e6)
    ref = PLBertTrainer(_cfg(), 188, max_batch=2, max_seq=32, lr=1e-3, state_dict=sd)
    assert ref.param_groups is None and [g["weight_decay"] for g in tr.param_groups] == [0.01, 0.0]
    p0 = tr.engine.params.clone()
    tr.step(tr.stage_batch(lab, msk, lens, idx))
    ref.step(ref.stage_batch(lab, msk, lens, idx))
    torch.cuda.synchronize()
    eng = tr.engine
    for k, (off, size, _) in eng.layout.items():
        sl = slice(off, off + size)
        if "embeddings." in k or "pooler" in k:
            assert torch.equal(eng.params[sl], p0[sl]) and k not in tr.stepped, k
            assert not bool(eng.exp_avg[sl].any())
        else:
            assert k in tr.stepped and (not k.endswith(".weight") or not torch.equal(eng.params[sl], p0[sl])), k
    # a decayed weight equals the default trainer's (same gradient, same settings, coefficient 1)
    off, size, _ = eng.layout["encoder.encoder.albert_layer_groups.0.albert_layers.0.ffn.weight"]
    assert float(tr.last_grad_norm[1]) == 1.0
    assert torch.equal(eng.params[off:off + size], ref.engine.params[off:off + size])
    # ... a bias does not: no decay
    off, size, _ = eng.layout["encoder.encoder.albert_layer_groups.0.albert_layers.0.ffn.bias"]
    assert not torch.equal(eng.params[off:off + size], ref.engine.params[off:off + size])
    assert rel_l2(eng.params[off:off + size], ref.engine.params[off:off + size]) < 1e-4
    assert eng.status()["ln_exchange_timeouts"] == 0


def _launches(tr, batch):
    tr.step(batch)                                   # warm: weight copies are in place, nothing left to sync
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    try:
        _lib.profile_read()
        tr.step(batch)
        torch.cuda.synchronize()
        return {k: v["launches"] for k, v in _lib.profile_read().items()}
    finally:
        _lib.profile_enable(False)


def test_default_trainer_launches_are_unchanged_by_the_group_entry_points():
    sd = plbert_amd.deterministic_state_dict(_cfg(), 188, seed=8)
    lab, msk, lens, idx = _ragged2(41)
    mk = lambda **kw: PLBertTrainer(_cfg(), 188, max_batch=2, max_seq=32, lr=1e-3, state_dict=sd, **kw)
    fresh = mk()
    base = _launches(fresh, fresh.stage_batch(lab, msk, lens, idx))
    used = mk()
    batch = used.stage_batch(lab, msk, lens, idx)
    used.loss_and_grads(batch)                       # every new entry point once, then the default step again
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    used.engine.adamw_plan(1, [hyper], [0] * NPARAM)
    nb = used.engine.grad_norm(1.0, 1.0, group_of=[0] * NPARAM)
    used.engine.adamw_step_groups(1, [hyper, hyper], [i % 2 for i in range(NPARAM)], norm_buf=nb)
    used.step_count = 1
    after = _launches(used, batch)
    assert after == base, (base, after)
    assert base.get("adamw") == 1 and sum(base.values()) > 20
    # the grouped trainer: still one AdamW launch, and nothing else added
    grouped = mk(no_decay=("bias", "LayerNorm"), frozen=("position_embeddings",))
    assert _launches(grouped, grouped.stage_batch(lab, msk, lens, idx)) == base


def test_checkpoint_carries_the_groups_and_a_resume_restores_them(tmp_path):
    from plbert_amd import run as R
    sd = plbert_amd.deterministic_state_dict(_cfg(), 188, seed=8)
    lab, msk, lens, idx = _ragged2(41)
    mk = lambda lr=1e-3, **kw: PLBertTrainer(_cfg(), 188, max_batch=2, max_seq=32, lr=lr, state_dict=sd, **kw)
    tr = mk(no_decay=("bias", "LayerNorm"), frozen=("position_embeddings",))
    batch = tr.stage_batch(lab, msk, lens, idx)
    tr.step(batch)
    tr.step(batch)
    path = R.save_checkpoint(tr, 2, str(tmp_path), 0)
    opt = torch.load(path, map_location="cpu", weights_only=False)["optimizer"]
    names = R.reference_param_names(tr.engine.layout)
    pos = names.index("encoder.embeddings.position_embeddings.weight")
    assert [g["weight_decay"] for g in opt["param_groups"]] == [0.01, 0.0] and all(g["lr"] == 1e-3 for g in opt["param_groups"])
    members = [i for g in opt["param_groups"] for i in g["params"]]
    assert pos not in members and len(members) == len(set(members)) == len(names) - 1
    assert pos not in opt["state"] and names.index("encoder.pooler.weight") not in opt["state"]    # never stepped: no state
    assert float(opt["state"][members[0]]["step"]) == 2.0
    # torch's own optimizer takes the entry (same group sizes) ...
    ps = [torch.nn.Parameter(torch.zeros(tr.engine.layout[n][2])) for n in names]
    tor = torch.optim.AdamW([{"params": [ps[i] for i in g["params"]]} for g in opt["param_groups"]], lr=9.0)
    tor.load_state_dict(opt)
    assert [g["weight_decay"] for g in tor.param_groups] == [0.01, 0.0]
    # ... and a resumed trainer continues exactly like the one that never stopped, groups and all
    again = mk()                                                                  # built without the arguments
    assert R.load_checkpoint(again, path) == 2 and again.step_count == 2
    assert [g["weight_decay"] for g in again.param_groups] == [0.01, 0.0]
    assert [sorted(g["names"]) for g in again.param_groups] == [sorted(g["names"]) for g in tr.param_groups]
    assert again.stepped == tr.stepped
    tr.step(batch)
    again.step(again.stage_batch(lab, msk, lens, idx))
    torch.cuda.synchronize()
    for what in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(tr.engine, what), getattr(again.engine, what)), what
    # the learning rate is the configuration's, as without groups: the file's 1e-3 does not come back
    slow = mk(lr=5e-4)
    R.load_checkpoint(slow, path)
    assert [g["lr"] for g in slow.groups_for_step()[0]] == [5e-4, 5e-4] and "lr" not in slow.param_groups[0]
    # a run configured with ANOTHER recipe does not resume from this file ...
    other = mk(no_decay=("bias",), frozen=("position_embeddings",))
    with pytest.raises(ValueError, match="other parameter groups"):
        R.load_checkpoint(other, path)
    # ... but may start from it as its pretrained model: the configured groups stay
    want = [sorted(g["names"]) for g in other.param_groups]
    R.load_checkpoint(other, path, restore_groups=False)
    assert [sorted(g["names"]) for g in other.param_groups] == want and other.step_count == 2
    # the same recipe resumes
    same = mk(no_decay=("bias", "LayerNorm"), frozen=("position_embeddings",))
    R.load_checkpoint(same, path)
    assert [sorted(g["names"]) for g in same.param_groups] == [sorted(g["names"]) for g in tr.param_groups]


def test_a_single_group_checkpoint_leaves_the_configured_groups_alone(tmp_path):
    """The file of an ungrouped run (the layout of a reference step_N.pth: one group over every parameter, with state) loaded
    into a trainer built with frozen= / no_decay=, as a resume and as a pretrained model: the embeddings stay frozen, the
    no-decay group stays, the learning rate stays the configuration's."""
    from plbert_amd import run as R
    sd = plbert_amd.deterministic_state_dict(_cfg(), 188, seed=8)
    lab, msk, lens, idx = _ragged2(41)
    mk = lambda **kw: PLBertTrainer(_cfg(), 188, max_batch=2, max_seq=32, state_dict=sd, **kw)
    plain = mk(lr=1e-3)
    plain.step(plain.stage_batch(lab, msk, lens, idx))
    path = R.save_checkpoint(plain, 1, str(tmp_path), 0)
    opt = torch.load(path, map_location="cpu", weights_only=False)["optimizer"]
    assert len(opt["param_groups"]) == 1 and opt["param_groups"][0]["lr"] == 1e-3 and len(opt["state"]) > 20
    for pretrained in (False, True):
        tr = mk(lr=5e-4, no_decay=("bias", "LayerNorm"), frozen=("embeddings.",))
        want = [(g["weight_decay"], sorted(g["names"])) for g in tr.param_groups]
        R.load_checkpoint(tr, path, restore_groups=not pretrained)
        assert [(g["weight_decay"], sorted(g["names"])) for g in tr.param_groups] == want and len(want) == 2
        assert not any("embeddings." in n for g in tr.param_groups for n in g["names"])
        assert [g["lr"] for g in tr.groups_for_step()[0]] == [5e-4, 5e-4] and tr.step_count == 1
        eng = tr.engine
        p0, m0 = eng.params.clone(), eng.exp_avg.clone()
        tr.step(tr.stage_batch(lab, msk, lens, idx))
        torch.cuda.synchronize()
        for k, (off, size, _) in eng.layout.items():
            sl = slice(off, off + size)
            if "embeddings." in k:                  # still frozen: parameters and the moments the file brought, bit for bit
                assert torch.equal(eng.params[sl], p0[sl]) and torch.equal(eng.exp_avg[sl], m0[sl]), k
                assert bool(m0[sl].any()), k
            elif k.endswith(".weight") and "pooler" not in k:
                assert not torch.equal(eng.params[sl], p0[sl]), k
        assert tr.step_count == 2
