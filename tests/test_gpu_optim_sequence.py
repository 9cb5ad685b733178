"""What every optimizer entry point launches, in every has-a-gradient state (-m gpu): per-kernel launch counts, the token
head's step count afterwards, the number of happens-before checks a call declares, and the "moved the weights" text a
step leaves for a stale plb_grad_accum_add. Engine of tests/test_gpu_grad_accum.py: embedding 64, hidden 128, 2 heads,
FFN 256, 2 layers, max_batch 4, max_seq 32, lengths [32, 19, 26, 11]; num_tokens 0 and 64.
States: after a phoneme-only loss call, after a dual-head loss call (num_tokens 64), after encode + encode_bwd (the phoneme
head has no gradient). Entries: plb_adamw_step, plb_adamw_step_clipped, plb_adamw_step_groups and plb_lamb_step (the last
two with and without a norm buffer; one frozen tensor, one no-decay group), plb_grad_norm, plb_grad_norm_groups, and
plb_grad_norm(have_partials) behind a window of two micro-steps.
The expected values are literals, recorded before the entry points were given one preamble and one range walk: they pin
which ranges are walked, where the token head's count advances and every HB_R / HB_W declaration. Values are not compared
here; that is tests/test_gpu_grad_accum.py, test_gpu_adamw_groups.py and test_gpu_lamb.py.
The four step entries' refusals behind "optimizer buffers not bound" need bound buffers: their order is asserted here too
(nothing is launched)."""
import ctypes as C

import numpy as np
import pytest
import torch

import plbert_amd
from plbert_amd import _lib
from plbert_amd.train import PLBertTrainer

pytestmark = pytest.mark.gpu

POSITION = "encoder.embeddings.position_embeddings.weight"
NO_DECAY = ("bias", "LayerNorm", "layer_norm")
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
STEPS = {"plain": "plb_adamw_step", "clipped": "plb_adamw_step_clipped", "groups": "plb_adamw_step_groups",
         "groups_norm": "plb_adamw_step_groups", "lamb": "plb_lamb_step", "lamb_norm": "plb_lamb_step"}
NORMS = ("norm", "norm_groups", "norm_partials")
STATES = [(0, "phoneme"), (0, "encode"), (64, "phoneme"), (64, "dual"), (64, "encode")]
TOK_STEPS_BEFORE = 5

# (num_tokens, state, entry) -> (launches per kernel class, token_head_steps afterwards, happens-before checks of the state's
# backward call(s) plus the entry)
EXPECT = {
    (0, 'phoneme', 'plain'): ({'adamw': 1, 'cast_transpose': 1}, 5, 29),
    (0, 'phoneme', 'clipped'): ({'reduce_slabs': 2, 'adamw': 1, 'cast_transpose': 1}, 5, 38),
    (0, 'phoneme', 'groups'): ({'adamw': 1, 'cast_transpose': 1}, 5, 29),
    (0, 'phoneme', 'groups_norm'): ({'reduce_slabs': 2, 'adamw': 1, 'cast_transpose': 1}, 5, 38),
    (0, 'phoneme', 'lamb'): ({'reduce_slabs': 1, 'adamw': 2, 'cast_transpose': 1}, 5, 29),
    (0, 'phoneme', 'lamb_norm'): ({'reduce_slabs': 3, 'adamw': 2, 'cast_transpose': 1}, 5, 38),
    (0, 'phoneme', 'norm'): ({'reduce_slabs': 2}, 5, 29),
    (0, 'phoneme', 'norm_groups'): ({'reduce_slabs': 2}, 5, 29),
    (0, 'phoneme', 'norm_partials'): ({'reduce_slabs': 2}, 5, 86),
    (0, 'encode', 'plain'): ({'adamw': 1, 'cast_transpose': 1}, 5, 30),
    (0, 'encode', 'clipped'): ({'reduce_slabs': 2, 'adamw': 1, 'cast_transpose': 1}, 5, 39),
    (0, 'encode', 'groups'): ({'adamw': 1, 'cast_transpose': 1}, 5, 30),
    (0, 'encode', 'groups_norm'): ({'reduce_slabs': 2, 'adamw': 1, 'cast_transpose': 1}, 5, 39),
    (0, 'encode', 'lamb'): ({'reduce_slabs': 1, 'adamw': 2, 'cast_transpose': 1}, 5, 30),
    (0, 'encode', 'lamb_norm'): ({'reduce_slabs': 3, 'adamw': 2, 'cast_transpose': 1}, 5, 39),
    (0, 'encode', 'norm'): ({'reduce_slabs': 2}, 5, 30),
    (0, 'encode', 'norm_groups'): ({'reduce_slabs': 2}, 5, 30),
    (0, 'encode', 'norm_partials'): ({'reduce_slabs': 2}, 5, 98),
    (64, 'phoneme', 'plain'): ({'adamw': 1, 'cast_transpose': 1}, 5, 29),
    (64, 'phoneme', 'clipped'): ({'reduce_slabs': 2, 'adamw': 1, 'cast_transpose': 1}, 5, 38),
    (64, 'phoneme', 'groups'): ({'adamw': 1, 'cast_transpose': 1}, 5, 29),
    (64, 'phoneme', 'groups_norm'): ({'reduce_slabs': 2, 'adamw': 1, 'cast_transpose': 1}, 5, 38),
    (64, 'phoneme', 'lamb'): ({'reduce_slabs': 1, 'adamw': 2, 'cast_transpose': 1}, 5, 29),
    (64, 'phoneme', 'lamb_norm'): ({'reduce_slabs': 3, 'adamw': 2, 'cast_transpose': 1}, 5, 38),
    (64, 'phoneme', 'norm'): ({'reduce_slabs': 2}, 5, 29),
    (64, 'phoneme', 'norm_groups'): ({'reduce_slabs': 2}, 5, 29),
    (64, 'phoneme', 'norm_partials'): ({'reduce_slabs': 2}, 5, 86),
    (64, 'dual', 'plain'): ({'adamw': 2, 'cast_transpose': 1}, 6, 29),
    (64, 'dual', 'clipped'): ({'reduce_slabs': 3, 'adamw': 2, 'cast_transpose': 1}, 6, 38),
    (64, 'dual', 'groups'): ({'adamw': 2, 'cast_transpose': 1}, 6, 29),
    (64, 'dual', 'groups_norm'): ({'reduce_slabs': 3, 'adamw': 2, 'cast_transpose': 1}, 6, 38),
    (64, 'dual', 'lamb'): ({'reduce_slabs': 2, 'adamw': 4, 'cast_transpose': 1}, 6, 29),
    (64, 'dual', 'lamb_norm'): ({'reduce_slabs': 5, 'adamw': 4, 'cast_transpose': 1}, 6, 38),
    (64, 'dual', 'norm'): ({'reduce_slabs': 3}, 5, 29),
    (64, 'dual', 'norm_groups'): ({'reduce_slabs': 3}, 5, 29),
    (64, 'dual', 'norm_partials'): ({'reduce_slabs': 3}, 5, 86),
    (64, 'encode', 'plain'): ({'adamw': 1, 'cast_transpose': 1}, 5, 30),
    (64, 'encode', 'clipped'): ({'reduce_slabs': 2, 'adamw': 1, 'cast_transpose': 1}, 5, 39),
    (64, 'encode', 'groups'): ({'adamw': 1, 'cast_transpose': 1}, 5, 30),
    (64, 'encode', 'groups_norm'): ({'reduce_slabs': 2, 'adamw': 1, 'cast_transpose': 1}, 5, 39),
    (64, 'encode', 'lamb'): ({'reduce_slabs': 1, 'adamw': 2, 'cast_transpose': 1}, 5, 30),
    (64, 'encode', 'lamb_norm'): ({'reduce_slabs': 3, 'adamw': 2, 'cast_transpose': 1}, 5, 39),
    (64, 'encode', 'norm'): ({'reduce_slabs': 2}, 5, 30),
    (64, 'encode', 'norm_groups'): ({'reduce_slabs': 2}, 5, 30),
    (64, 'encode', 'norm_partials'): ({'reduce_slabs': 2}, 5, 98),
}


def _cfg():
    return plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)


def _ragged(seed, lengths, S=32):
    labels, masked, _, idx = plbert_amd.synthetic_batch(len(lengths), S, seed=seed)
    out = []
    for b, n in enumerate(lengths):
        out.append([i for i in idx[b] if i < n] or [n // 2])
        labels[b, n:] = 0
        masked[b, n:] = 0
    return labels, masked, np.asarray(lengths, np.int32), out


class Rig:
    """One warm trainer per num_tokens, shared by the cases: every case sets its own state up with fresh backward calls."""

    def __init__(self, num_tokens):
        sd = plbert_amd.deterministic_state_dict(_cfg(), 188, num_tokens, seed=8)
        self.tr = PLBertTrainer(_cfg(), 188, max_batch=4, max_seq=32, lr=1e-3, state_dict=sd, num_tokens=num_tokens)
        self.eng = self.tr.engine
        lab, msk, lens, idx = _ragged(41, [32, 19, 26, 11])
        self.mono = self.tr.stage_batch(lab, msk, lens, idx)
        self.dual = None
        if num_tokens:
            tok = np.random.RandomState(5).randint(0, num_tokens, size=lab.shape).astype(np.int64)
            self.dual = self.tr.stage_batch(lab, msk, lens, idx, token_ids=tok)
        self.ids, self.lens = np.random.RandomState(3).randint(1, 180, size=(4, 32)), lens
        self.d_hidden = torch.randn(4, 32, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
        names = list(self.eng.layout)
        self.group_of = {n: int(any(x in n for x in NO_DECAY)) for n in names if n != POSITION}
        self.groups = [dict(HYPER, weight_decay=0.01), dict(HYPER, weight_decay=0.0)]
        self.lamb_groups = [dict(g, adapt=k == 0) for k, g in enumerate(self.groups)]
        self.tr.step(self.mono)                  # warm: the weight copies are in place, the buffers exist
        self.eng.grad_norm(1.0, 1.0)
        self.eng.lamb_buf
        torch.cuda.synchronize()

    def backward(self, state):
        if state == "encode":
            self.eng.encode(self.ids, self.lens)
            self.eng.encode_bwd(self.d_hidden)
        else:
            self.tr.loss_and_grads(self.dual if state == "dual" else self.mono)

    def run(self, entry, step):
        eng = self.eng
        if entry in NORMS:
            gof = self.group_of if entry == "norm_groups" else None
            return eng.grad_norm(0.5, 1.0, have_partials=entry == "norm_partials", group_of=gof)
        nb = eng.grad_norm(0.5, 1.0, group_of=None if entry == "clipped" else self.group_of) if entry.endswith("norm") or \
            entry == "clipped" else None
        if entry in ("plain", "clipped"):
            return eng.adamw_step(step, weight_decay=0.01, grad_scale=0.5, norm_buf=nb, **HYPER)
        if entry.startswith("groups"):
            return eng.adamw_step_groups(step, self.groups, self.group_of, grad_scale=0.5, norm_buf=nb)
        return eng.lamb_step(step, self.lamb_groups, self.group_of, grad_scale=0.5, norm_buf=nb)


_rigs = {}


@pytest.fixture
def rig(request):
    nt = request.param
    if nt not in _rigs:
        _rigs[nt] = Rig(nt)
    return _rigs[nt]


def _measure(rig, state, entry):
    eng = rig.eng
    eng.token_head_steps = TOK_STEPS_BEFORE
    eng.hb_audit(True)
    try:
        rig.backward(state)
        if entry == "norm_partials":             # a window of two micro-steps
            eng.grad_accum_add(eng.GRAD_FIRST)
            rig.backward(state)
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        try:
            _lib.profile_read()
            if entry == "norm_partials":
                eng.grad_accum_add(eng.GRAD_LAST, want_partials=True)
            rig.run(entry, 3)
            torch.cuda.synchronize()
            launches = {k: v["launches"] for k, v in _lib.profile_read().items()}
        finally:
            _lib.profile_enable(False)
        rep = eng.hb_report()
    finally:
        eng.hb_audit(False)
    assert rep["violations"] == 0, rep
    return launches, eng.token_head_steps, rep["checks"]


@pytest.mark.parametrize("entry", list(STEPS) + list(NORMS))
@pytest.mark.parametrize("rig,state", STATES, indirect=["rig"])
def test_entry_launches_steps_and_declares_what_it_did(rig, state, entry):
    nt = rig.eng.num_tokens
    got = _measure(rig, state, entry)
    print(f"    ({nt}, {state!r}, {entry!r}): {got!r},")
    assert got == EXPECT[(nt, state, entry)]
    assert rig.eng.status()["ln_exchange_timeouts"] == 0


@pytest.mark.parametrize("entry", list(STEPS))
@pytest.mark.parametrize("rig,state", STATES, indirect=["rig"])
def test_a_step_names_itself_to_a_stale_add(rig, state, entry):
    eng = rig.eng
    rig.backward(state)
    eng.grad_accum_add(eng.GRAD_FIRST)
    rig.run(entry, 4)
    with pytest.raises(RuntimeError) as err:
        eng.grad_accum_add(eng.GRAD_ADD)
    assert str(err.value) == "plb_grad_accum_add failed: plb_grad_accum_add: phase 1 without a FIRST add: no window is open " \
                             f"({STEPS[entry]} moved the weights)"
    torch.cuda.synchronize()


@pytest.mark.parametrize("rig", [0, 64], indirect=True)
def test_refusal_order_of_the_step_entries_on_bound_buffers(rig):
    """Behind "optimizer buffers not bound" (tests/test_optim_refusals_host.py): the entry's own refusals, in its order.
    Nothing is launched; the window a FIRST add opened is still open afterwards."""
    eng, L, h = rig.eng, rig.eng.L, rig.eng.handle
    rig.backward("phoneme")
    eng.grad_accum_add(eng.GRAD_FIRST)
    nb, lb, odd = eng.norm_buf.data_ptr(), eng.lamb_buf.data_ptr(), eng.lamb_buf.data_ptr() + 4
    n = _lib.PLB_NPARAM

    def refused(rc):
        assert rc != 0
        return L.plb_last_error().decode()

    assert refused(L.plb_adamw_step(h, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0, 1.0, None)) == "plb_adamw_step: step counts from 1"
    who = "plb_adamw_step_clipped"
    assert refused(L.plb_adamw_step_clipped(h, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0, 1.0, None, None)) == f"{who}: step counts from 1"
    assert refused(L.plb_adamw_step_clipped(h, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 1.0, None, None)) == \
        f"{who}: norm_buf is null (plb_grad_norm writes it)"
    ok, bad_gof = (C.c_int32 * n)(), (C.c_int32 * n)(*([0, 3] + [0] * (n - 2)))
    good = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
    for who, fn, mk, tail in (
            ("plb_adamw_step_groups", L.plb_adamw_step_groups, lambda g: _lib.PlbAdamWGroup(*g.values()), (nb, None)),
            ("plb_lamb_step", L.plb_lamb_step, lambda g: _lib.PlbLambGroup(*g.values(), g.get("adapt", 1)), (nb, lb, None))):
        arr = lambda *gs: (type(mk(good)) * len(gs))(*[mk(g) for g in gs])
        bad = arr(dict(good, lr=-1.0, beta2=1.0))
        assert refused(fn(h, None, 0, None, 0, 1.0, *tail)) == f"{who}: group_of is null"
        assert refused(fn(h, None, 0, ok, 0, 1.0, *tail)) == f"{who}: n_groups 0: there must be at least one group"
        assert refused(fn(h, bad, 1, bad_gof, 0, 1.0, *tail)) == f"{who}: group_of[1] = 3 is outside [-1, 1)"
        assert refused(fn(h, None, 1, ok, 0, 1.0, *tail)) == f"{who}: groups is null"
        assert refused(fn(h, bad, 1, ok, 0, 1.0, *tail)) == f"{who}: group 0: lr -1 is negative or not finite"
        assert refused(fn(h, arr(good, dict(good, beta2=1.0)), 2, ok, 0, 1.0, *tail)) == f"{who}: group 1: beta2 1 is outside [0, 1)"
        assert refused(fn(h, arr(good), 1, ok, 0, 1.0, *tail)) == f"{who}: step counts from 1"
    g = lambda **kw: (_lib.PlbLambGroup * 1)(_lib.PlbLambGroup(1e-3, 0.9, 0.999, 1e-8, kw.get("wd", 0.01), kw.get("adapt", 1)))
    who = "plb_lamb_step"
    assert refused(L.plb_lamb_step(h, g(wd=float("inf"), adapt=2), 1, ok, 0, 1.0, nb, None, None)) == \
        f"{who}: group 0: weight_decay is not finite"
    assert refused(L.plb_lamb_step(h, g(adapt=2), 1, ok, 0, 1.0, nb, None, None)) == f"{who}: group 0: adapt 2 is neither 0 nor 1"
    for buf in (None, odd):
        assert refused(L.plb_lamb_step(h, g(), 1, ok, 0, 1.0, nb, buf, None)) == f"{who}: step counts from 1"
        assert refused(L.plb_lamb_step(h, g(), 1, ok, 1, 1.0, nb, buf, None)) == \
            f"{who}: lamb_buf must be a 16-byte aligned device buffer"
    rig.backward("phoneme")
    eng.grad_accum_add(eng.GRAD_LAST)            # no refused call closed the window
    torch.cuda.synchronize()
