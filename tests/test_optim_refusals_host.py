"""Every refusal of the optimizer entry points that can be reached without a device, with its complete text and, where two
apply at once, which one reports (include/plbert.h: plb_adamw_step, plb_adamw_step_clipped, plb_adamw_step_groups,
plb_lamb_step, plb_grad_norm, plb_grad_norm_groups, plb_grad_accum_bind, plb_grad_accum_add, plb_adamw_plan, plb_lamb_plan).
The engine is created and never bound (tests/test_adamw_groups_host.py: embedding 64, hidden 128, 2 heads, FFN 256, 2 layers,
max_batch 2, max_seq 32), num_tokens 0 and 64, plus an inference-only one. Every case returns before a launch: the device
pointers are made-up addresses that nothing dereferences. The texts are literals, recorded before the entry points were
given one preamble and one range walk.
On a never bound engine the four step entries stop at "optimizer buffers not bound", their first refusal, which also shadows
"inference-only engine" (such an engine binds no gradient or moment buffer). What follows it (the step count, the groups,
lamb_buf) needs bound buffers and is asserted in tests/test_gpu_optim_sequence.py."""
import ctypes as C

import pytest

from plbert_amd import _lib

N = _lib.PLB_NPARAM
FAKE = C.c_void_p(1 << 20)            # 16-byte aligned, never dereferenced
ODD = C.c_void_p((1 << 20) + 4)       # not 16-byte aligned
ADAMW = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
LAMB = dict(ADAMW, adapt=1)
NAN, INF = float("nan"), float("inf")


class Created:
    """plb_create without a device."""

    def __init__(self, num_tokens=0, inference_only=0):
        self.L = _lib.lib()
        c = _lib.PlbConfig(188, 64, 128, 2, 256, 2, 512, 2, 1e-12, 188, num_tokens, 2, 32, inference_only)
        self.h = C.c_void_p()
        assert self.L.plb_create(C.byref(c), C.byref(self.h)) == 0

    def __del__(self):
        self.L.plb_destroy(self.h)


def _refused(L, rc):
    assert rc != 0
    return L.plb_last_error().decode()


def _gof(*values):
    v = list(values) + [0] * (N - len(values))
    return (C.c_int32 * N)(*v)


def _adamw_groups(*groups):
    return (_lib.PlbAdamWGroup * max(1, len(groups)))(*[_lib.PlbAdamWGroup(g["lr"], g["beta1"], g["beta2"], g["eps"],
                                                                           g["weight_decay"]) for g in groups])


def _lamb_groups(*groups):
    return (_lib.PlbLambGroup * max(1, len(groups)))(*[_lib.PlbLambGroup(g["lr"], g["beta1"], g["beta2"], g["eps"],
                                                                         g["weight_decay"], g["adapt"]) for g in groups])


@pytest.fixture(params=[0, 64])
def eng(request):
    return Created(request.param)


# ---- the four step entries: bound first, whatever else is wrong ------------------------------------------------------------
def _step_calls(L, h, step=1, norm=FAKE, lamb=FAKE, gof=None, groups=True):
    gof = _gof() if gof is None else gof
    return {
        "plb_adamw_step": lambda: L.plb_adamw_step(h, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 1.0, None),
        "plb_adamw_step_clipped": lambda: L.plb_adamw_step_clipped(h, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 1.0, norm, None),
        "plb_adamw_step_groups": lambda: L.plb_adamw_step_groups(h, _adamw_groups(ADAMW) if groups else None, 1, gof, step,
                                                                 1.0, norm, None),
        "plb_lamb_step": lambda: L.plb_lamb_step(h, _lamb_groups(LAMB) if groups else None, 1, gof, step, 1.0, norm, lamb, None),
    }


@pytest.mark.parametrize("entry", ["plb_adamw_step", "plb_adamw_step_clipped", "plb_adamw_step_groups", "plb_lamb_step"])
def test_step_entries_report_unbound_buffers_before_anything_else(eng, entry):
    L = eng.L
    want = f"{entry}: optimizer buffers not bound"
    assert _refused(L, _step_calls(L, None)[entry]()) == want                       # a null engine has no buffers either
    assert _refused(L, _step_calls(L, eng.h)[entry]()) == want
    # ... before inference-only, a bad step, a null norm_buf / lamb_buf, null or bad groups
    inf = Created(0, inference_only=1)
    assert _refused(L, _step_calls(L, inf.h)[entry]()) == want
    assert _refused(L, _step_calls(L, eng.h, step=0)[entry]()) == want
    assert _refused(L, _step_calls(L, eng.h, norm=None, lamb=None)[entry]()) == want
    assert _refused(L, _step_calls(L, eng.h, norm=ODD, lamb=ODD)[entry]()) == want
    assert _refused(L, _step_calls(L, eng.h, gof=_gof(-2), groups=False)[entry]()) == want


# ---- plb_grad_norm, plb_grad_norm_groups -----------------------------------------------------------------------------------
def test_grad_norm_refusals_and_their_order(eng):
    L, h = eng.L, eng.h
    inf = Created(0, inference_only=1)
    assert _refused(L, L.plb_grad_norm(None, 1.0, 1.0, FAKE, 0, None)) == "plb_grad_norm: null engine"
    assert _refused(L, L.plb_grad_norm(inf.h, 1.0, 1.0, FAKE, 0, None)) == "plb_grad_norm: inference-only engine"
    assert _refused(L, L.plb_grad_norm(inf.h, 1.0, 1.0, None, 1, None)) == "plb_grad_norm: inference-only engine"
    buf = "plb_grad_norm: norm_buf must be a 16-byte aligned device buffer"
    assert _refused(L, L.plb_grad_norm(h, 1.0, 1.0, None, 0, None)) == buf
    assert _refused(L, L.plb_grad_norm(h, 1.0, 1.0, ODD, 0, None)) == buf
    assert _refused(L, L.plb_grad_norm(h, 1.0, 1.0, ODD, 1, None)) == buf           # before have_partials
    assert _refused(L, L.plb_grad_norm(h, 1.0, 1.0, FAKE, 1, None)) == \
        "plb_grad_norm: have_partials, but the last plb_grad_accum_add(LAST) left none in this buffer"   # before "not bound"
    assert _refused(L, L.plb_grad_norm(h, 1.0, 1.0, FAKE, 0, None)) == "plb_grad_norm: gradient buffer not bound"


def test_grad_norm_groups_refusals_and_their_order(eng):
    L, h = eng.L, eng.h
    who = "plb_grad_norm_groups"
    inf = Created(0, inference_only=1)
    ok = _gof()
    assert _refused(L, L.plb_grad_norm_groups(None, ok, 1.0, 0.0, FAKE, None)) == f"{who}: null engine"
    assert _refused(L, L.plb_grad_norm_groups(inf.h, None, 1.0, 0.0, None, None)) == f"{who}: inference-only engine"
    assert _refused(L, L.plb_grad_norm_groups(h, None, 1.0, 0.0, None, None)) == f"{who}: group_of is null"
    assert _refused(L, L.plb_grad_norm_groups(h, _gof(-2), 1.0, 0.0, None, None)) == \
        f"{who}: group_of[0] = -2 is outside [-1, 1073741824)"                      # before the norm buffer
    assert _refused(L, L.plb_grad_norm_groups(h, _gof(0, 0, 1 << 30), 1.0, 0.0, FAKE, None)) == \
        f"{who}: group_of[2] = 1073741824 is outside [-1, 1073741824)"
    buf = f"{who}: norm_buf must be a 16-byte aligned device buffer"
    assert _refused(L, L.plb_grad_norm_groups(h, ok, 1.0, 0.0, None, None)) == buf
    assert _refused(L, L.plb_grad_norm_groups(h, _gof(-1, 5), 1.0, 0.0, ODD, None)) == buf
    assert _refused(L, L.plb_grad_norm_groups(h, ok, 1.0, 0.0, FAKE, None)) == f"{who}: gradient buffer not bound"


# ---- plb_grad_accum_bind, plb_grad_accum_add -------------------------------------------------------------------------------
def test_grad_accum_refusals_and_their_order(eng):
    L, h = eng.L, eng.h
    who = "plb_grad_accum_add"
    inf = Created(0, inference_only=1)
    assert _refused(L, L.plb_grad_accum_bind(None, FAKE)) == "plb_grad_accum_bind: null engine"
    assert _refused(L, L.plb_grad_accum_bind(None, ODD)) == "plb_grad_accum_bind: null engine"
    assert _refused(L, L.plb_grad_accum_bind(h, ODD)) == "plb_grad_accum_bind: the buffer must be 16-byte aligned"
    assert _refused(L, L.plb_grad_accum_add(None, 0, None, None)) == f"{who}: null engine"
    assert _refused(L, L.plb_grad_accum_add(inf.h, 7, ODD, None)) == f"{who}: inference-only engine"
    unbound = f"{who}: no accumulation buffer bound (plb_grad_accum_bind)"
    assert _refused(L, L.plb_grad_accum_add(h, 0, None, None)) == unbound
    assert _refused(L, L.plb_grad_accum_add(h, 3, ODD, None)) == unbound             # before the phase and norm_buf
    assert L.plb_grad_accum_bind(h, FAKE) == 0
    assert _refused(L, L.plb_grad_accum_add(h, 3, FAKE, None)) == f"{who}: phase 3 is none of 0 (first), 1 (add), 2 (last)"
    assert _refused(L, L.plb_grad_accum_add(h, -1, None, None)) == f"{who}: phase -1 is none of 0 (first), 1 (add), 2 (last)"
    last = f"{who}: partial sums belong to the LAST add (phase 2)"
    assert _refused(L, L.plb_grad_accum_add(h, 0, FAKE, None)) == last
    assert _refused(L, L.plb_grad_accum_add(h, 1, ODD, None)) == last                # before the alignment, before the window
    assert _refused(L, L.plb_grad_accum_add(h, 2, ODD, None)) == f"{who}: norm_buf must be 16-byte aligned"   # before the window
    for phase in (1, 2):
        assert _refused(L, L.plb_grad_accum_add(h, phase, None, None)) == \
            f"{who}: phase {phase} without a FIRST add: no window is open (no FIRST add has opened one)"
    assert _refused(L, L.plb_grad_accum_add(h, 0, None, None)) == \
        f"{who}: the gradient buffer holds nothing new: no backward call has run since the last add (the same gradients " \
        "would be added twice)"
    assert L.plb_grad_accum_bind(h, None) == 0                                       # unbinding brings the first text back
    assert _refused(L, L.plb_grad_accum_add(h, 1, None, None)) == unbound


# ---- plb_adamw_plan, plb_lamb_plan -----------------------------------------------------------------------------------------
def _plan(L, who, h, groups, n_groups, gof, step, out=True):
    lamb = who == "plb_lamb_plan"
    garr = None if groups is None else (_lamb_groups if lamb else _adamw_groups)(*groups)
    segs = ((_lib.PlbLambSegment if lamb else _lib.PlbAdamWSegment) * N)() if out else None
    n = C.c_int32(-1)
    return getattr(L, who)(h, garr, n_groups, gof, step, segs, C.byref(n) if out else None)


@pytest.mark.parametrize("who", ["plb_adamw_plan", "plb_lamb_plan"])
def test_plan_refusals_and_their_order(eng, who):
    L, h = eng.L, eng.h
    g = LAMB                                                                         # (the AdamW form ignores adapt)
    ok = _gof()
    inf = Created(0, inference_only=1)
    bad = dict(g, lr=-1.0)
    # group_of first
    assert _refused(L, _plan(L, who, None, [g], 1, ok, 1)) == f"{who}: null engine"
    assert _refused(L, _plan(L, who, h, None, 0, None, 0, out=False)) == f"{who}: group_of is null"
    assert _refused(L, _plan(L, who, h, None, 0, ok, 0, out=False)) == f"{who}: n_groups 0: there must be at least one group"
    assert _refused(L, _plan(L, who, h, None, -3, ok, 1)) == f"{who}: n_groups -3: there must be at least one group"
    assert _refused(L, _plan(L, who, h, [bad], 1, _gof(0, 0, 0, 1), 0)) == f"{who}: group_of[3] = 1 is outside [-1, 1)"
    assert _refused(L, _plan(L, who, h, [g, g], 2, _gof(1, -2, 7), 1)) == f"{who}: group_of[1] = -2 is outside [-1, 2)"
    # then the groups, in the order lr, eps, beta1, beta2, weight_decay (, adapt), group by group, then the step count
    assert _refused(L, _plan(L, who, h, None, 1, ok, 0, out=False)) == f"{who}: groups is null"
    for key, value, text in (("lr", -1e-3, "lr -0.001 is negative or not finite"), ("lr", INF, "lr inf is negative or not finite"),
                             ("lr", NAN, "lr nan is negative or not finite"), ("eps", -1e-8, "eps -1e-08 is negative or not finite"),
                             ("eps", NAN, "eps nan is negative or not finite"), ("eps", INF, "eps inf is negative or not finite"),
                             ("beta1", 1.0, "beta1 1 is outside [0, 1)"), ("beta1", -0.1, "beta1 -0.1 is outside [0, 1)"),
                             ("beta1", NAN, "beta1 nan is outside [0, 1)"), ("beta2", 1.0, "beta2 1 is outside [0, 1)"),
                             ("beta2", -0.5, "beta2 -0.5 is outside [0, 1)"), ("beta2", NAN, "beta2 nan is outside [0, 1)"),
                             ("weight_decay", INF, "weight_decay is not finite"), ("weight_decay", NAN, "weight_decay is not finite")):
        assert _refused(L, _plan(L, who, h, [dict(g, **{key: value})], 1, ok, 1)) == f"{who}: group 0: {text}"
        assert _refused(L, _plan(L, who, h, [g, dict(g, **{key: value})], 2, ok, 0, out=False)) == f"{who}: group 1: {text}"
    all_bad = dict(lr=-1.0, eps=-1.0, beta1=2.0, beta2=2.0, weight_decay=NAN, adapt=2)
    order = [("lr", "lr -1 is negative or not finite"), ("eps", "eps -1 is negative or not finite"),
             ("beta1", "beta1 2 is outside [0, 1)"), ("beta2", "beta2 2 is outside [0, 1)"),
             ("weight_decay", "weight_decay is not finite")]
    if who == "plb_lamb_plan":
        order.append(("adapt", "adapt 2 is neither 0 nor 1"))
    cur = dict(all_bad)
    for key, text in order:
        assert _refused(L, _plan(L, who, h, [cur], 1, ok, 0)) == f"{who}: group 0: {text}"
        cur = dict(cur, **{key: g[key]})
    assert _refused(L, _plan(L, who, h, [dict(g, lr=-2.0), bad], 2, ok, 1)) == f"{who}: group 0: lr -2 is negative or not finite"
    if who == "plb_lamb_plan":
        assert _refused(L, _plan(L, who, h, [dict(g, adapt=-1)], 1, ok, 1)) == f"{who}: group 0: adapt -1 is neither 0 nor 1"
        assert _plan(L, who, h, [dict(g, adapt=0)], 1, ok, 1) == 0
    else:
        assert _plan(L, who, h, [dict(g, adapt=2)], 1, ok, 1) == 0                   # no such field in PlbAdamWGroup
    assert _refused(L, _plan(L, who, h, [g], 1, ok, 0, out=False)) == f"{who}: step counts from 1"
    assert _refused(L, _plan(L, who, h, [g], 1, ok, -5)) == f"{who}: step counts from 1"
    # then the outputs, and the inference-only engine last
    assert _refused(L, _plan(L, who, h, [g], 1, ok, 1, out=False)) == f"{who}: null output"
    assert _refused(L, _plan(L, who, inf.h, [g], 1, ok, 1, out=False)) == f"{who}: null output"
    assert _refused(L, _plan(L, who, inf.h, [g], 1, ok, 1)) == f"{who}: inference-only engine"
    assert _refused(L, _plan(L, who, inf.h, [bad], 1, ok, 1)) == f"{who}: group 0: lr -1 is negative or not finite"
    assert _plan(L, who, h, [dict(g, beta1=0.0, beta2=0.0, lr=0.0, eps=0.0)], 1, _gof(*([-1] * N)), 1) == 0   # the closed ends
