"""The AdamW element contract proved on the CPU (no GPU): gpu_util.adamw_fp64 / check_adamw, the instrument that
tests/test_gpu_adamw_elements.py holds plb_launch_adamw and plb_launch_adamw_clipped to.

 - The allowance is not tight by construction: a numpy float32 restatement of adamw_kernel's operation list — once unfused,
   once with g gs - m as one fused operation, the contraction hipcc makes — stays at or below 0.75 of each allowance at every
   (lr, wd, grad_scale) x step of the GPU module, on 65536 elements of the same state.
 - The instrument catches what it is for: each planted defect in the restatement is named with its first offending element.
 - The gap it closes: defects 5 to 8 keep rel_l2 of the parameters against the reference below 1e-6, the bound of
   tests/test_gpu_adamw_kernel.py."""
import numpy as np
import pytest

import gpu_util as gu

N = 65536
HOST_LIMIT = 0.75


@pytest.fixture(scope="module")
def state():
    return gu.adamw_state(N)


def _rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def test_the_state_has_its_special_elements(state):
    p, g, m, v = state
    assert all(a.dtype == np.float32 and a.shape == (N,) for a in state)
    assert (p[::53] == 0).all() and (g[::97] == 0).all() and (m[::31] == 0).all() and (v[::41] == 0).all()
    assert int((np.abs(p) > 100).sum()) > 100 and int((v == np.float32(1e-30)).sum()) > 500
    still = (g == 0) & (m == 0) & (v == 0)
    assert int(still.sum()) >= N // 211 and int((still & (p != 0)).sum()) > 200
    for n in (4, 1020, 1028):   # a short range is the same generator, not a prefix: it still has zeros of every kind
        q = gu.adamw_state(n)
        assert q[0].shape == (n,) and q[0][0] == 0 and q[1][0] == 0


@pytest.mark.parametrize("step", gu.ADAMW_STEPS)
@pytest.mark.parametrize("lr,wd,gs", gu.ADAMW_TRIPLES + (gu.ADAMW_DECAY_TRIPLE,))
def test_the_restatement_uses_at_most_three_quarters_of_each_allowance(state, lr, wd, gs, step):
    ref = gu.adamw_fp64(*state, lr, wd, gs, step)
    for fused in (False, True):
        got = gu.adamw_f32_restatement(*state, lr, wd, gs, step, fused=fused)
        ratios = gu.check_adamw(f"fused={fused}", *got, ref, limit=HOST_LIMIT)
        assert max(ratios.values()) <= HOST_LIMIT and min(ratios.values()) > 0.05, ratios   # neither tight nor idle


@pytest.mark.parametrize("coef", [1.0, 0.37])
def test_the_clipped_form_uses_at_most_three_quarters(state, coef):
    for (lr, wd, gs), step in zip(gu.ADAMW_TRIPLES, (1, 10, 100000)):
        ref = gu.adamw_fp64(*state, lr, wd, gs, step, coef=np.float32(coef))
        got = gu.adamw_f32_restatement(*state, lr, wd, gs, step, coef=np.float32(coef))
        gu.check_adamw(f"coef={coef}", *got, ref, limit=HOST_LIMIT)


def _offender(state, got, lr, wd, gs, step):
    ref = gu.adamw_fp64(*state, lr, wd, gs, step)
    _, off = gu.adamw_offender(*got, ref)
    with pytest.raises(AssertionError) if off is not None else _NoRaise():
        gu.check_adamw("planted", *got, ref)
    return ref, off


class _NoRaise:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _first_bad(state, got, ref):
    """The first index per array at which `got` differs from the clean restatement by more than the allowance: what the
    checker has to name (computed independently of adamw_offender's own loop)."""
    out = {}
    for name, a, want, tol in (("m", got[1], ref.m, ref.tol_m), ("v", got[2], ref.v, ref.tol_v), ("p", got[0], ref.p, ref.tol_p)):
        bad = np.flatnonzero(np.abs(a.astype(np.float64) - want) > tol)
        if bad.size:
            out[name] = int(bad[0])
    return out


@pytest.mark.parametrize("lr,wd,gs", gu.ADAMW_TRIPLES)
def test_defect_1_one_minus_beta2_formed_in_float32_is_flagged_on_v(state, lr, wd, gs):
    got = gu.adamw_f32_restatement(*state, lr, wd, gs, 10, defect="omb2")
    ref, off = _offender(state, got, lr, wd, gs, 10)
    assert off is not None and off[0] == "v" and off[1] == _first_bad(state, got, ref)["v"]
    # 1.0f - 0.999f is 1.3e-5 off: far over 8u wherever the gradient term carries v'
    assert abs(off[2] - off[3]) > 10 * off[4]


@pytest.mark.parametrize("step", [1, 2, 10])
def test_defect_2_bias_correction_from_the_next_step(state, step):
    lr, wd, gs = gu.ADAMW_TRIPLES[0]
    got = gu.adamw_f32_restatement(*state, lr, wd, gs, step, defect="step+1")
    ref, off = _offender(state, got, lr, wd, gs, step)
    assert off is not None and off[0] == "p" and off[1] == _first_bad(state, got, ref)["p"]   # m and v do not see it


@pytest.mark.parametrize("defect", ["no_sqrt_bc2", "eps_inside"])
@pytest.mark.parametrize("step", [1, 10, 1000])
def test_defects_3_and_4_the_denominator(state, defect, step):
    lr, wd, gs = gu.ADAMW_TRIPLES[1]
    got = gu.adamw_f32_restatement(*state, lr, wd, gs, step, defect=defect)
    ref, off = _offender(state, got, lr, wd, gs, step)
    assert off is not None and off[0] == "p" and off[1] == _first_bad(state, got, ref)["p"]


@pytest.mark.parametrize("step", gu.ADAMW_STEPS)
def test_defect_5_decay_after_the_update(state, step):
    lr, wd, gs = gu.ADAMW_DECAY_TRIPLE
    got = gu.adamw_f32_restatement(*state, lr, wd, gs, step, defect="decay_after")
    ref, off = _offender(state, got, lr, wd, gs, step)
    assert off is not None and off[0] == "p" and off[1] == _first_bad(state, got, ref)["p"]
    assert _rel_l2(got[0], ref.p) < 1e-6                      # the whole-range norm does not see it


def test_why_m_and_v_share_their_exponent():
    """With m and v drawn independently |m| / sqrt(v) reaches 10^7: the updated range is made of updates, not of
    parameters, and a whole-range norm DOES see the misplaced decay. Such a state would hide the gap, not show it."""
    lr, wd, gs = gu.ADAMW_DECAY_TRIPLE
    loose = gu.adamw_state(N, shared_exponent=False)
    ref = gu.adamw_fp64(*loose, lr, wd, gs, 10)
    assert float(np.abs(ref.upd).max()) > 1e4 * lr
    got = gu.adamw_f32_restatement(*loose, lr, wd, gs, 10, defect="decay_after")
    assert _rel_l2(got[0], ref.p) > 1e-4
    tight = gu.adamw_fp64(*gu.adamw_state(N), lr, wd, gs, 10)
    assert float(np.abs(tight.upd).max()) < 100 * lr


@pytest.mark.parametrize("lr,wd,gs", gu.ADAMW_TRIPLES + (gu.ADAMW_DECAY_TRIPLE,))
def test_defect_6_the_last_float4_left_unupdated(state, lr, wd, gs):
    got = [a.copy() for a in gu.adamw_f32_restatement(*state, lr, wd, gs, 3, fused=True)]
    p, g, m, v = state
    for a, old in zip(got, (p, m, v)):
        a[-4:] = old[-4:]
    ref, off = _offender(state, got, lr, wd, gs, 3)
    assert off is not None and off[1] >= N - 4 and off[1] == _first_bad(state, got, ref)[off[0]]
    assert _rel_l2(got[0], ref.p) < 1e-6


def test_defect_7_two_components_of_one_float4_swapped(state):
    lr, wd, gs = gu.ADAMW_TRIPLES[0]
    got = [a.copy() for a in gu.adamw_f32_restatement(*state, lr, wd, gs, 3)]
    p = got[0].reshape(-1, 4)
    gap = np.abs(p[:, 2].astype(np.float64) - p[:, 3])
    k = int(np.flatnonzero((gap > 1e-4) & (gap < 1e-3))[0])   # two neighbours that differ by 10^3 allowances, and by
    for a in got:                                             # 10^-7 of the range's norm
        a[4 * k + 2], a[4 * k + 3] = a[4 * k + 3], a[4 * k + 2]
    ref, off = _offender(state, got, lr, wd, gs, 3)
    assert off is not None and off[1] in (4 * k + 2, 4 * k + 3)
    assert _first_bad(state, got, ref)["p"] == 4 * k + 2
    assert _rel_l2(got[0], ref.p) < 1e-6


def test_defect_8_one_bf16_copy_truncated(state):
    lr, wd, gs = gu.ADAMW_TRIPLES[0]
    p1, m1, v1 = gu.adamw_f32_restatement(*state, lr, wd, gs, 3)
    bits = gu.bf16_rne_bits(p1)
    gu.check_bf16_copy("clean", bits, p1)
    trunc = (p1.view(np.uint32) >> 16).astype(np.uint16)
    k = int(np.flatnonzero(trunc != bits)[N // 2 // 3])       # an element the two roundings disagree on
    bad = bits.copy()
    bad[k] = trunc[k]
    with pytest.raises(AssertionError, match=r"bf16 copy \[%d\]" % k):
        gu.check_bf16_copy("planted", bad, p1)
    as_f32 = lambda b: (b.astype(np.uint32) << 16).view(np.float32)   # noqa: E731
    ref = gu.adamw_fp64(*state, lr, wd, gs, 3)
    assert _rel_l2(as_f32(bad), as_f32(bits)) < 1e-6 and _rel_l2(p1, ref.p) < 1e-6


def test_bf16_rounding_is_nearest_even_and_the_tie_values_are_ties():
    import torch
    x = gu.bf16_tie_values()
    assert np.isfinite(x).all() and (x > 0).any() and (x < 0).any()
    bits = gu.bf16_rne_bits(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(bits, want)
    low = x.view(np.uint32) & 0xFFFF
    ties = low == 0x8000
    assert int(ties.sum()) == x.size // 3
    up = bits[ties] != (x.view(np.uint32)[ties] >> 16)
    assert up.any() and (~up).any()                            # ties to even go both ways
    assert ((bits[ties] & 1) == 0).all()
    r = np.random.RandomState(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(gu.bf16_rne_bits(r), torch.from_numpy(r).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_a_zero_second_moment_must_come_back_exactly_zero(state):
    lr, wd, gs = gu.ADAMW_TRIPLES[0]
    ref = gu.adamw_fp64(*state, lr, wd, gs, 2)
    got = [a.copy() for a in gu.adamw_f32_restatement(*state, lr, wd, gs, 2)]
    k = int(np.flatnonzero(ref.v == 0)[5])
    got[2][k] = np.float32(1e-38)
    _, off = gu.adamw_offender(*got, ref)
    assert off is not None and off[:2] == ("v", k)
    # and a parameter whose update is exactly zero must be p x decay to the bit
    got = [a.copy() for a in gu.adamw_f32_restatement(*state, lr, wd, gs, 2)]
    still = np.flatnonzero((ref.gj == 0) & (ref.m == 0) & (ref.v == 0) & (ref.p_in != 0))
    k = int(still[3])
    got[0][k] = np.nextafter(got[0][k], np.float32(np.inf))
    with pytest.raises(AssertionError, match=r"p\[%d\] has a zero update" % k):
        gu.check_adamw("planted", *got, ref)
