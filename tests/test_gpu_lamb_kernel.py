"""The LAMB kernels through their launchers (-m gpu): plb_launch_lamb_pass1 / _finish / _pass2 on synthetic flat buffers, against
plb_launch_adamw_clipped (the moments, bit for bit) and against the float64 restatement (tests/lamb_ref.py).

Layout: tensors of 4, 128, 128, 1020, 1024, 1028, 3 x 1024 + 4 and 4 x 1024 + 12 floats with a hole of 8 floats behind the
third: a tensor shorter than a wave, tensors shorter than a workgroup's piece of 1024 floats, a boundary one float4 either side
of 1024, a tensor whose last piece holds one float4, and one of 5 pieces (the multi-partial sum). Values from randn, scaled per
tensor over 1e-3 ... 1e+2. Every buffer lies between guards and the hole and the guards hold NaN sentinels.

Bounds (EPS = 2^-24, the unit roundoff of fp32; first order, constants rounded up — none is fitted to a run).
 * A partial sum: every term is a square, the product inside each fused multiply-add is exact, so only additions round; the
   longest chain behind one partial is PLB_LAMB_CHAIN = 4 (a thread's own) + 6 (wave) + 3 (four waves) = 13 additions:
   relative error <= 13 EPS. The partials of a tensor are added in double (negligible). The square root halves it, the
   conversion of the double root to fp32 adds EPS:   |wn_gpu - wn| <= (13 / 2 + 1 + 0.5) EPS wn = 8 EPS wn   (0.5: second order).
 * un adds the error of u itself. With g' = fl(fl(g gs) coef) (2 EPS), A = |m| + (1 - beta1)(|g'| + |m|) the size of the terms m'
   is made of, and den = sqrt(v') / sqrt(bc2) + eps:  |dm'| <= 3 EPS A;  v' has three roundings on top of g'^2 (4 EPS): 7 EPS,
   its root 3.5 + 0.5, the division and the sum one each: den to 6 EPS;  r = m' / den: |dr| <= 7 EPS |r| + 3 EPS A / den;
   u = fma(r, 1 / bc1, fl(wd p)):  |du| <= EPS [ (7 |r| + 3 A / den) / bc1 + |wd p| + |u| ] =: EPS e_i.
   |un_gpu - un| <= EPS ||e|| + 8 EPS un.
 * trust = fl(wn / un): rel(wn) + rel(un) + EPS = (17 + ||e|| / un) EPS; ||e|| / un is 11 to 13 on these inputs (printed), so about
   30 EPS = 1.8e-6: the tolerance of 1e-5 set for trust has more than 5x headroom, and both are asserted.
 * p, element by element: |p_gpu - p_f64| <= ulp(p) / 2 + lr trust |u| (1e-5 + 4 EPS).
 * The bf16 copy equals the rounding of the stored p exactly; m, v equal plb_launch_adamw_clipped's bit for bit."""
import numpy as np
import pytest
import torch

import gpu_util as gu
import lamb_ref as R
from gpu_util import stream
from plbert_amd import _lib

pytestmark = pytest.mark.gpu

NPARAM = _lib.PLB_NPARAM
PAD = 64
SENT_F32, SENT_BF16 = 0x7FC0ABCD, 0x7FC1
SIZES = (4, 128, 128, 1020, 1024, 1028, 3 * 1024 + 4, 4 * 1024 + 12)
HOLE_AFTER, HOLE = 2, 8
GS = 0.125
EPS = R.EPS
HYPER = ((1e-3, (0.9, 0.999), 1e-6, 0.01, 1), (2e-3, (0.8, 0.99), 1e-8, 0.0, 7), (5e-4, (0.95, 0.98), 1e-6, 0.1, 1000))
SLOTS = (0, 1, 3, 4, 7, 8, 20, 28)          # result slots: increasing, with gaps (the slots between are holes of the results)


def _bounds():
    out, at = [], 0
    for k, n in enumerate(SIZES):
        out.append((at, at + n))
        at += n + (HOLE if k == HOLE_AFTER else 0)
    return out, at


BOUNDS, N = _bounds()


def _tensors(adapt=None, wd=None):
    ts = []
    for k, (a, b) in enumerate(BOUNDS):
        lr, betas, eps, w, step = HYPER[k % len(HYPER)]
        ts.append(R.tensor(a, b, lr, betas, eps, w if wd is None or wd[k] is None else wd[k], step,
                           1 if adapt is None else adapt[k], SLOTS[k], k % 2))
    return ts


def _segs(tensors):
    arr = (_lib.PlbLambSegment * max(1, len(tensors)))()
    for k, t in enumerate(tensors):
        arr[k] = _lib.PlbLambSegment(t["begin"], t["end"], t["tensor"], t["group"], t["step"], t["adapt"],
                                     *[t[key] for key in R.SCALARS])
    return arr


@pytest.fixture(scope="module")
def state():
    """p, g, m, v as float32 numpy arrays of N floats: randn, every tensor on a scale of its own."""
    gen = torch.Generator().manual_seed(2025)
    p, g, m, v = (np.zeros(N, np.float32) for _ in range(4))
    scales = np.logspace(-3, 2, len(BOUNDS))
    for k, (a, b) in enumerate(BOUNDS):
        sp, sg = scales[k], scales[::-1][k]
        r = lambda: torch.randn(b - a, generator=gen).numpy().astype(np.float64)
        p[a:b] = (r() * sp).astype(np.float32)
        g[a:b] = (r() * sg / GS).astype(np.float32)
        m[a:b] = (r() * sg * 0.3).astype(np.float32)
        v[a:b] = ((r() * sg) ** 2 * 0.5 + (0.1 * sg) ** 2).astype(np.float32)
    return p, g, m, v


class Buffers:
    """p, g, m, v (fp32 bit patterns) and the bf16 copy of N floats between guards; guards and the hole hold sentinels."""

    def __init__(self, state):
        live = np.zeros(N, dtype=bool)
        for a, b in BOUNDS:
            live[a:b] = True
        self.live = live
        self.t = {}
        for name, a in zip("pgmv", state):
            buf = torch.full((PAD + N + PAD,), SENT_F32, dtype=torch.int32)
            bits = torch.from_numpy(a.view(np.int32).copy())
            buf[PAD:PAD + N] = torch.where(torch.from_numpy(live), bits, torch.tensor(SENT_F32, dtype=torch.int32))
            self.t[name] = buf.cuda()
        self.t["b"] = torch.full((PAD + N + PAD,), SENT_BF16, dtype=torch.int16, device="cuda")
        self.results = torch.full((4 * NPARAM,), -7.0, device="cuda")
        self.partials = torch.full((2 * 64,), -7.0, device="cuda")

    def ptr(self, name):
        return self.t[name].data_ptr() + PAD * self.t[name].element_size()

    def f32(self, name):
        return self.t[name][PAD:PAD + N].cpu().numpy().view(np.float32)

    def same_bits(self, other, what, names="pgmvb"):
        for k in names:
            assert torch.equal(self.t[k], other.t[k]), f"{what}: {k} differs (guards and the hole included)"


def _lamb(bufs, tensors, norm=None, skip=None, count_skip=0, count_nonfinite=0, gs=GS):
    """The three launches of one range, as plb_lamb_step issues them."""
    L = _lib.lib()
    segs, n = _segs(tensors), len(tensors)
    wgs = L.plb_lamb_workgroups(segs, n, N)
    assert wgs == sum((b - a + 1023) // 1024 for a, b in BOUNDS) and 2 * wgs <= bufs.partials.numel()
    sk = skip.data_ptr() if skip is not None else None
    nm = norm.data_ptr() if norm is not None else None
    assert L.plb_launch_lamb_pass1(bufs.ptr("p"), bufs.ptr("g"), bufs.ptr("m"), bufs.ptr("v"), N, segs, n, gs, sk, count_skip, nm,
                                   count_nonfinite, bufs.partials.data_ptr(), stream()) == 0
    assert L.plb_launch_lamb_finish(segs, n, N, 0, NPARAM, bufs.partials.data_ptr(), bufs.results.data_ptr(), sk, nm, stream()) == 0
    assert L.plb_launch_lamb_pass2(bufs.ptr("p"), bufs.ptr("m"), bufs.ptr("v"), bufs.ptr("b"), N, segs, n, bufs.results.data_ptr(),
                                   sk, nm, stream()) == 0
    torch.cuda.synchronize()
    return bufs.results.cpu().numpy().reshape(NPARAM, 4)


@pytest.fixture(scope="module")
def stepped(state):
    """One step per coefficient (None: no norm buffer), shared by the tests that only read it: (buffers, results, reference)."""
    out = {}
    for coef in (None, 1.0, 0.37):
        bufs = Buffers(state)
        norm = None if coef is None else torch.tensor([5.0, coef, 0.0, 2.0], dtype=torch.float32, device="cuda")
        res = _lamb(bufs, _tensors(), norm=norm, count_nonfinite=1)
        if norm is not None:
            assert norm.tolist() == [5.0, float(np.float32(coef)), 0.0, 2.0]               # a finite norm: nothing is counted
        out[coef] = (bufs, res, R.lamb_ref(*state, _tensors(), GS, coef))
    return out


# ---- 1. the moments are the clipped AdamW's ----------------------------------------------------------------------------------
@pytest.mark.parametrize("coef", [None, 1.0, 0.37])
def test_moments_equal_the_clipped_adamw_bit_for_bit(state, stepped, coef):
    L = _lib.lib()
    got = stepped[coef][0]
    want = Buffers(state)
    norm = torch.tensor([5.0, 1.0 if coef is None else coef, 0.0, 0.0], dtype=torch.float32, device="cuda")
    for (a, b), t in zip(BOUNDS, _tensors()):
        lr, betas, eps, wd, step = HYPER[BOUNDS.index((a, b)) % len(HYPER)]
        ptrs = [want.ptr(k) + a * (2 if k == "b" else 4) for k in "pgmvb"]
        assert L.plb_launch_adamw_clipped(*ptrs, b - a, lr, betas[0], betas[1], eps, wd, step, GS, None, 0, norm.data_ptr(), 0,
                                          stream()) == 0
    torch.cuda.synchronize()
    got.same_bits(want, f"coef={coef}", names="mvg")
    fresh = Buffers(state)
    assert torch.equal(got.t["g"], fresh.t["g"])                                           # the gradient is only read
    live = torch.from_numpy(np.pad(got.live, PAD)).cuda()
    for k in "pmvb":                                                                       # guards and the hole: untouched
        changed = got.t[k] != fresh.t[k]
        assert not bool(changed[~live].any()), k
        assert float(changed[live].float().mean()) > 0.5, k


# ---- 2. norms and trust ratios ---------------------------------------------------------------------------------------------
def _u_error_terms(state, tensors, coef, ref):
    """e_i of the docstring, float64."""
    p, g, m, v = (np.asarray(x, np.float64) for x in state)
    e = np.zeros(N)
    for t in tensors:
        sl = slice(t["begin"], t["end"])
        gg = np.abs(g[sl]) * GS * (1.0 if coef is None else float(np.float32(coef)))
        A = np.abs(m[sl]) + t["omb1"] * (gg + np.abs(m[sl]))
        den = np.sqrt(ref["v"][sl]) / t["bc2_sqrt"] + t["eps"]
        r = np.abs(ref["m"][sl]) / den
        e[sl] = (7 * r + 3 * A / den) * t["inv_bc1"] + np.abs(t["weight_decay"] * p[sl]) + np.abs(ref["u"][sl])
    return e


@pytest.mark.parametrize("coef", [None, 1.0, 0.37])
def test_norms_and_trust_against_float64(state, stepped, coef):
    _, res, ref = stepped[coef]
    tensors = _tensors()
    e = _u_error_terms(state, tensors, coef, ref)
    chain = (_lib.LAMB_CHAIN / 2 + 1.5) * EPS
    for k, t in enumerate(tensors):
        wn, un, trust, live = (float(x) for x in res[t["tensor"]])
        e_norm = float(np.sqrt(np.sum(e[t["begin"]:t["end"]] ** 2)))
        b_wn, b_un = chain, chain + EPS * e_norm / ref["un"][k]
        b_trust = b_wn + b_un + EPS
        rel = lambda got, want: abs(got - want) / want
        print(f"tensor {k} ({t['end'] - t['begin']} floats) coef={coef}: wn {rel(wn, ref['wn'][k]) / EPS:.2f} EPS (bound {b_wn / EPS:.1f}), "
              f"un {rel(un, ref['un'][k]) / EPS:.2f} EPS (bound {b_un / EPS:.1f}), trust {rel(trust, ref['trust'][k]) / EPS:.2f} EPS "
              f"(bound {b_trust / EPS:.1f}; 1e-5 = {1e-5 / EPS:.0f} EPS)")
        assert live == 1.0
        assert rel(wn, ref["wn"][k]) <= b_wn, (k, "wn")
        assert rel(un, ref["un"][k]) <= b_un, (k, "un")
        assert rel(trust, ref["trust"][k]) <= min(b_trust, R.TRUST_RTOL), (k, "trust")
        assert b_trust < R.TRUST_RTOL / 3                                                  # the headroom the docstring claims
    holes = [s for s in range(NPARAM) if s not in SLOTS]
    assert not res[holes].any()                                                            # [0, 0, 0, live = 0]


# ---- 3. the parameters, element by element -----------------------------------------------------------------------------------
@pytest.mark.parametrize("coef", [None, 1.0, 0.37])
def test_parameters_element_by_element(state, stepped, coef):
    bufs, res, ref = stepped[coef]
    p = bufs.f32("p").astype(np.float64)
    worst = 0.0
    for k, t in enumerate(_tensors()):
        sl = slice(t["begin"], t["end"])
        bound = R.p_bound(ref["p"][sl], ref["u"][sl], t["lr"], ref["trust"][k])
        ratio = np.abs(p[sl] - ref["p"][sl]) / bound
        i = int(np.argmax(ratio))
        print(f"tensor {k} coef={coef}: worst |p_gpu - p_f64| / bound = {ratio[i]:.3f} at {i} (p = {ref['p'][sl][i]:.6g}, "
              f"u = {ref['u'][sl][i]:.6g}, lr trust = {t['lr'] * ref['trust'][k]:.4g})")
        worst = max(worst, float(ratio[i]))
        assert ratio[i] <= 1.0, (k, i)
        assert float(np.mean(p[sl] != np.asarray(state[0], np.float64)[sl])) > 0.5          # it moved
    live = bufs.live
    gu.check_bf16_copy(f"bf16 copy, coef={coef}", bufs.t["b"][PAD:PAD + N].cpu().numpy().view(np.uint16)[live], bufs.f32("p")[live])


# ---- 4. edge cases -----------------------------------------------------------------------------------------------------------
def test_zero_tensor_zero_update_and_adapt_off(state):
    p, g, m, v = (x.copy() for x in state)
    (a1, b1), (a2, b2), (a3, b3) = BOUNDS[1], BOUNDS[2], BOUNDS[5]
    p[a1:b1] = 0.0                                                  # an all-zero tensor: wn = 0
    g[a2:b2] = 0.0; m[a2:b2] = 0.0; v[a2:b2] = 0.0                  # zero gradient and zero decay on zero moments: un = 0
    wd = [None] * len(BOUNDS); wd[2] = 0.0
    adapt = [1] * len(BOUNDS); adapt[5] = 0                         # and a tensor of an adapt = 0 group
    tensors = _tensors(adapt, wd)
    bufs = Buffers((p, g, m, v))
    res = _lamb(bufs, tensors)
    ref = R.lamb_ref(p, g, m, v, tensors, GS)
    got_p = bufs.f32("p")
    assert np.isfinite(got_p[bufs.live]).all() and np.isfinite(res).all()
    wn, un, trust, live = res[SLOTS[1]]
    assert wn == 0.0 and trust == 1.0 and un > 0.0 and live == 1.0
    sl = slice(a1, b1)                                              # p = 0 - lr * 1 * u
    assert (np.abs(got_p[sl] - ref["p"][sl]) <= R.p_bound(ref["p"][sl], ref["u"][sl], tensors[1]["lr"], 1.0)).all()
    assert np.count_nonzero(got_p[sl]) > 100
    wn, un, trust, live = res[SLOTS[2]]
    assert un == 0.0 and trust == 1.0 and wn > 0.0 and live == 1.0
    assert np.array_equal(got_p[a2:b2].view(np.uint32), p[a2:b2].view(np.uint32))           # nothing to apply
    assert not bufs.f32("m")[a2:b2].any() and not bufs.f32("v")[a2:b2].any()
    wn, un, trust, live = res[SLOTS[5]]
    assert trust == 1.0 and wn > 0.0 and un > 0.0 and abs(wn / un - 1.0) > 0.1              # the ratio would not have been 1
    sl = slice(a3, b3)
    assert (np.abs(got_p[sl] - ref["p"][sl]) <= R.p_bound(ref["p"][sl], ref["u"][sl], tensors[5]["lr"], 1.0)).all()
    # guards and the hole of p, m, v and the bf16 copy still hold their sentinels
    pad_live = np.pad(bufs.live, PAD)
    for k in "pmv":
        assert bool((bufs.t[k].cpu().numpy()[~pad_live] == np.int32(SENT_F32)).all()), k
    assert bool((bufs.t["b"].cpu().numpy().view(np.uint16)[~pad_live] == SENT_BF16).all())
    gu.check_bf16_copy("bf16 copy", bufs.t["b"][PAD:PAD + N].cpu().numpy().view(np.uint16)[bufs.live], got_p[bufs.live])


# ---- 5. the skip word and the non-finite flag ----------------------------------------------------------------------------------
@pytest.mark.parametrize("clipped", [False, True])
def test_skip_word_and_nonfinite_flag_store_nothing_and_count_once(state, clipped):
    bufs, fresh = Buffers(state), Buffers(state)
    norm = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float32, device="cuda") if clipped else None
    for count_skip in (0, 1, 2):
        skip = torch.tensor([3, 10, 20, 30], dtype=torch.int32, device="cuda")     # a caller-owned word, set by a copy
        for k in range(2):
            _lamb(bufs, _tensors(), norm=norm, skip=skip, count_skip=count_skip, count_nonfinite=1)
            want = [3, 10, 20, 30]
            if count_skip:
                want[count_skip] += k + 1                                            # exactly one per step of three launches
            assert skip.tolist() == want
    bufs.same_bits(fresh, "skip[0] != 0")                                           # m and v are not advanced either
    assert torch.equal(bufs.results, fresh.results) and torch.equal(bufs.partials, fresh.partials)
    if clipped:
        assert norm.tolist() == [1.0, 1.0, 0.0, 0.0]                                # the skip word is tested first
        bad = torch.tensor([float("inf"), 0.0, 1.0, 2.0], dtype=torch.float32, device="cuda")
        skip = torch.tensor([0, 10, 20, 30], dtype=torch.int32, device="cuda")
        _lamb(bufs, _tensors(), norm=bad, skip=skip, count_skip=1, count_nonfinite=1)
        assert bad.tolist()[2:] == [1.0, 3.0]
        _lamb(bufs, _tensors(), norm=bad, skip=skip, count_skip=1, count_nonfinite=0)
        assert bad.tolist()[2:] == [1.0, 3.0] and skip.tolist() == [0, 10, 20, 30]
        bufs.same_bits(fresh, "norm[2] != 0")
        assert torch.equal(bufs.results, fresh.results) and torch.equal(bufs.partials, fresh.partials)


# ---- 6. reproducible, and what the launchers refuse -----------------------------------------------------------------------------
def test_two_runs_from_the_same_state_give_the_same_bytes(state, stepped):
    first = stepped[0.37][0]
    again = Buffers(state)
    _lamb(again, _tensors(), norm=torch.tensor([5.0, 0.37, 0.0, 2.0], dtype=torch.float32, device="cuda"), count_nonfinite=1)
    again.same_bits(first, "second run")
    assert torch.equal(again.results.view(torch.int32), first.results.view(torch.int32))
    assert torch.equal(again.partials.view(torch.int32), first.partials.view(torch.int32))


def test_launcher_refusals_write_nothing(state):
    L = _lib.lib()
    bufs, fresh = Buffers(state), Buffers(state)
    good = _tensors()

    def refused(tensors, n=N):
        segs, k = _segs(tensors), len(tensors)
        rc1 = L.plb_launch_lamb_pass1(bufs.ptr("p"), bufs.ptr("g"), bufs.ptr("m"), bufs.ptr("v"), n, segs, k, GS, None, 0, None, 0,
                                      bufs.partials.data_ptr(), stream())
        rc2 = L.plb_launch_lamb_finish(segs, k, n, 0, NPARAM, bufs.partials.data_ptr(), bufs.results.data_ptr(), None, None, stream())
        rc3 = L.plb_launch_lamb_pass2(bufs.ptr("p"), bufs.ptr("m"), bufs.ptr("v"), bufs.ptr("b"), n, segs, k, bufs.results.data_ptr(),
                                      None, None, stream())
        return rc1 != 0 and rc2 != 0 and rc3 != 0 and L.plb_lamb_workgroups(segs, k, n) == -1

    edit = lambda k, **kw: good[:k] + [{**good[k], **kw}] + good[k + 1:]
    assert refused(edit(3, adapt=2)) and refused(edit(3, adapt=-1))                 # adapt is 0 or 1
    assert refused(edit(3, begin=good[3]["begin"] + 2))                             # a boundary that is no multiple of 4
    assert refused(edit(3, begin=good[3]["begin"] - 12))                            # overlapping (behind the hole)
    assert refused(edit(3, end=good[3]["begin"]))                                   # empty
    assert refused(edit(7, end=N + 4))                                              # beyond n
    assert refused(edit(3, tensor=good[2]["tensor"]))                               # slots must increase
    assert refused(edit(7, tensor=NPARAM))                                          # ... inside [0, PLB_NPARAM)
    assert refused(edit(3, step=0))
    assert refused(good, n=N + 2)
    assert refused(good * 4)                                                        # more than PLB_NPARAM (and unsorted)
    assert L.plb_launch_lamb_finish(_segs(good), len(good), N, 1, NPARAM, bufs.partials.data_ptr(), bufs.results.data_ptr(), None, None,
                                    stream()) != 0                                  # a tensor outside the finish's slots
    torch.cuda.synchronize()
    bufs.same_bits(fresh, "refused")
    assert torch.equal(bufs.results, fresh.results) and torch.equal(bufs.partials, fresh.partials)
