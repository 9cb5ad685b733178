"""No GPU: the attention row contract (gpu_util.check_rows / check_delta) checks itself on the CPU.

tests/test_gpu_attention_rows.py holds every (token row, head) of the kernels' ctx, dq, dk and dv to the float64 reference
within 4 x the worst row of the rounding model. Here the model's own outputs stand in for a kernel's (B = 2, S = 65,
NH = 1, lengths 65 and 40), first untouched, then with a defect in ONE row:

  * the model sits within its own bound, and its per-output maxima are printed (-s);
  * one row scaled until its error is 5 x the model's maximum: the row check fails and names the row, while the aggregate
    limits of test_gpu_kernels.py (rel_l2 < 6e-3 for ctx, < 1.5e-2 for dq / dk / dv) still pass on the same tensor;
  * one query row recomputed without its last valid key: the row check fails;
  * delta of one row off by 1e-3 of its absolute sum: the delta check fails.

Measured on the CPU (maximum row error of attention_rounded against attention_fp64 | aggregate rel_l2 of the tensor with the
5 x defect in row 7):

    output   model max   4 x bound   aggregate, model   aggregate, one row at 5 x   aggregate limit
    ctx      2.672e-03   1.069e-02   2.099e-03          2.381e-03                   6e-3
    dq       3.625e-03   1.450e-02   2.435e-03          4.249e-03                   1.5e-2
    dk       3.646e-03   1.458e-02   2.419e-03          2.729e-03                   1.5e-2
    dv       3.416e-03   1.366e-02   2.239e-03          2.561e-03                   1.5e-2
  dropped key: probability 9.4e-03 in row 45, caught in ctx and dq.
"""
import pytest
import torch

from gpu_util import (ROW_FACTOR, attention_delta_terms, attention_fp64, attention_rounded, check_delta, check_rows, rel_l2)

B, S, NH = 2, 65, 1
H = NH * 64
LENS = [65, 40]
ROW = 7                                    # the row that gets the defect: valid in both samples' outputs
AGGREGATE = {"ctx": 6e-3, "dq": 1.5e-2, "dk": 1.5e-2, "dv": 1.5e-2}   # the limits of tests/test_gpu_kernels.py


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(301)
    qkv = torch.randn(B * S, 3 * H, generator=g).to(torch.bfloat16)
    lengths = torch.tensor(LENS, dtype=torch.int32)
    inside = (torch.arange(S)[None, :] < lengths[:, None]).reshape(B * S)
    dctx = (torch.randn(B * S, H, generator=g) * inside[:, None]).to(torch.bfloat16)
    ref, mod = {}, {}
    for out, fn in ((ref, attention_fp64), (mod, attention_rounded)):
        out["ctx"], out["lse"], grad = fn(qkv, lengths, B, S, NH)
        out["dq"], out["dk"], out["dv"], out["delta"] = grad(dctx)
    valid = {"ctx": None, "dq": inside, "dk": inside, "dv": inside}
    return dict(qkv=qkv, lengths=lengths, inside=inside, dctx=dctx, ref=ref, mod=mod, valid=valid)


def rows(case, name, got):
    return check_rows(name, got, case["ref"][name], case["mod"][name], NH, valid=case["valid"][name])


def test_model_within_its_own_bound(case):
    for name in AGGREGATE:
        st = rows(case, name, case["mod"][name])
        print(f"host rows {name}: model max {st['model']:.3e}, bound {st['bound']:.3e}, aggregate "
              f"{rel_l2(case['mod'][name], case['ref'][name]):.3e}")
        assert 0.0 < st["model"] == st["got"] <= st["bound"] and st["n_abs"] == 0
    # the model keeps the exact log-sum-exp and rounds the stored statistic inside its backward
    assert torch.equal(case["mod"]["lse"], case["ref"]["lse"])


@pytest.mark.parametrize("name", list(AGGREGATE))
def test_one_row_defect_is_caught_by_rows_and_missed_by_the_aggregate(case, name):
    ref, mod = case["ref"][name], case["mod"][name]
    worst = rows(case, name, mod)["model"]
    got = mod.clone()
    got[ROW] = ref[ROW] * (1.0 + 5.0 * worst)       # the row's error is now 5 x the model's maximum: just over the 4 x bound
    assert 5.0 > ROW_FACTOR
    with pytest.raises(AssertionError, match=rf"{name}: row {ROW} head 0 "):
        rows(case, name, got)
    agg = rel_l2(got, ref)
    print(f"host rows {name}: defect of {5.0 * worst:.3e} in row {ROW} caught; aggregate {agg:.3e} < {AGGREGATE[name]:g}")
    assert agg < AGGREGATE[name]


def test_dropped_key_is_caught(case):
    """One query row of sample 0 evaluated without key 64, the last valid one. A key is worth what its probability is, so
    the row is the TYPICAL one: the query for which that key has the median probability of the 65 (about 1 %)."""
    x = case["qkv"][:S].double()
    p_last = torch.softmax(x[:, :H] @ x[:, H:2 * H].T * 0.125, dim=-1)[:, S - 1]
    row = int(p_last.argsort()[S // 2])
    short = case["lengths"].clone()
    short[0] -= 1
    ctx, _, grad = attention_rounded(case["qkv"], short, B, S, NH)
    dq = grad(case["dctx"])[0]
    for name, t in (("ctx", ctx), ("dq", dq)):
        got = case["mod"][name].clone()
        got[row] = t[row]
        with pytest.raises(AssertionError, match=rf"{name}: row {row} head 0 "):
            rows(case, name, got)
        print(f"host rows {name}: key of probability {float(p_last[row]):.3e} dropped from row {row}: caught")


def test_biased_delta_is_caught(case):
    ref, mag = attention_delta_terms(case["dctx"], case["mod"]["ctx"], B, S, NH)
    assert torch.allclose(case["mod"]["delta"], ref, rtol=0, atol=1e-12)
    assert torch.equal(attention_fp64(case["qkv"], case["lengths"], B, S, NH)[2](case["dctx"], case["mod"]["ctx"])[3], ref)
    got = ref.float()                               # as the kernel stores it
    check_delta(got, ref, mag)
    got[0, 0, ROW] += 1e-3 * float(mag[0, 0, ROW])
    with pytest.raises(AssertionError, match=rf"delta\[0, 0, {ROW}\]"):
        check_delta(got, ref, mag)


def test_degenerate_and_padded_rows_are_counted(case):
    """A row may leave the relative check only as predicted: a zeroed valid row is a count mismatch, a padded row must be 0."""
    got = case["mod"]["dq"].clone()
    ref = case["ref"]["dq"].clone()
    ref[ROW] = 0.0
    with pytest.raises(AssertionError, match="1 .* fall under the absolute check, 0 predicted"):
        check_rows("dq", got, ref, case["mod"]["dq"], NH, valid=case["inside"])
    got[S + LENS[1]] = 1e-3                          # the first padded query of sample 1
    with pytest.raises(AssertionError, match=f"padded row {S + LENS[1]} "):
        rows(case, "dq", got)
