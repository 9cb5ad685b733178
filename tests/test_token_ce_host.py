"""CPU proof of the instrument of tests/test_gpu_token_ce.py (no GPU): token_ce_ref's restatement of the fused token-head
cross-entropy is inside every allowance on every case of the table, its checker catches AND locates nine seeded defects,
and the aggregate that held this path so far (rel_l2 < 4e-3 on the gradient, allclose(rtol 2e-5) on the loss rows:
test_gpu_kernels.py::test_fused_gemm_cross_entropy_passes) is shown, with its measured values, to miss some of them on the
same data. Run with -s for the fractions and the aggregate's figures."""
import pytest
import torch

import token_ce_ref as R
from gpu_util import EXACT_LIMIT, rel_l2


made = R.made


def model(name, TM, defect=None):
    case, ops, _, _ = made(name)
    return R.restated(ops.A, ops.W, ops.bias, ops.tgt, case.lengths, case.B, case.S, case.ce_cols, TM, case.row_start,
                      defect=defect, exact=case.exact)


def aggregate(got, ref):
    """The two assertions of test_fused_gemm_cross_entropy_passes: (gradient rel_l2, loss rows allclose, whether both pass)."""
    cc = ref.ce_cols
    l2 = rel_l2(got.grad[:, :cc].float(), ref.grad[:, :cc].float())
    close = bool(torch.allclose(got.loss.double(), ref.loss, rtol=2e-5, atol=1e-7))
    return l2, close, (l2 < 4e-3 and close)


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_is_inside_every_allowance(name):
    case, ops, ref, allow = made(name)
    for form, TM in R.FORMS.items():
        rep = R.check(model(name, TM), ref, allow, ops.cls, case.exact)
        for out, v in rep.items():
            print(f"token-ce {name} form {form}: {out} model {v.frac:.4f} at {v.at}")
        assert not R.failures(rep), R.failures(rep)
    l2, close, ok = aggregate(model(name, 256), ref)
    assert ok, (l2, close)                                  # (the aggregate accepts the model too: its misses below mean something)


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c.exact])
def test_exactness_premise_holds_for_every_table_row(name):
    _, ops, ref, _ = made(name)
    assert R.premise(ops) < EXACT_LIMIT
    z32 = ref.z.float()
    assert torch.equal(z32.double(), ref.z)                 # every logit IS an fp32 number


@pytest.mark.parametrize("name", list(R.CASES))
def test_absolute_floor_counts_equal_the_designed_counts(name):
    """Elements below w 2^-100, counted from the reference: every class but the winner of a sharp row with a gap of 80 or
    128 (a losing target's element is -w and the winner's w; a winning target's own element w (1 - p) is below 2^-53 w,
    which float64 holds as 0) and none in the soft, tie, offset and gauss classes."""
    _, ops, ref, allow = made(name)
    assert R.floor_count(ref) == ops.floor_designed == int(allow.floor.sum())
    per_row = allow.floor.sum(1)
    for r in range(R.M):
        if not ops.cls[r].startswith(("sharp80", "sharp128")):
            assert int(per_row[r]) == 0, (r, ops.cls[r])
    assert (ops.floor_designed > 0) == R.CASES[name].exact


def row_of(name, cls, nth=0):
    return [r for r, c in enumerate(made(name)[1].cls) if c == cls][nth]


def first_w0(name):
    return int((~made(name)[1].valid).nonzero()[0])


# (defect, case, row argument, output that must report it, (row, column tile) where the first report must be; None = any)
DEFECTS = {
    "softmax*1.03": ("n256c200", lambda: row_of("n256c200", "soft/t=any", 1), "grad"),
    "onehot+1": ("n256c200", lambda: row_of("n256c200", "soft/t=strip31", 1), "grad"),
    "neighbour_lse": ("gauss", lambda: 6, "grad"),
    "cols+1": ("n512c300", lambda: 0, "psum"),
    "drop": ("n16640c16500", lambda: row_of("n16640c16500", "soft/t=any", 1), "lse"),
    "norescale": ("n16640c16500", lambda: row_of("n16640c16500", "sharp32@second/t=winner", 1), "lse"),
    "0*exp(inf)": ("n256c200", lambda: first_w0("n256c200"), "grad"),
    "colpart-64": ("n256c200", lambda: 1, "colpart"),
    "tie_not_top1": ("n512c512", lambda: 0, "top1"),
}


def seeded(defect):
    name, rowf, out = DEFECTS[defect]
    case, ops, ref, allow = made(name)
    row = rowf()
    got = model(name, 256, (defect, row))
    rep = R.check(got, ref, allow, ops.cls, case.exact)
    assert rep[out].bad > 0, f"defect {defect} was not caught"
    l2, close, ok = aggregate(got, ref)
    print(f"defect {defect} on {name} row {row}: {rep[out].first} | aggregate: gradient rel_l2 {l2:.3e}, loss rows allclose {close}"
          f" -> {'MISSED' if ok else 'seen'}")
    return row, rep, out, ok, l2


def test_softmax_scaled_by_1_03_in_one_row_is_located_and_the_aggregate_misses_it():
    """One row of 256: the aggregate's gradient rel_l2 reads 8.6e-4 (limit 4e-3; the rows' one-hot terms dominate the norm)
    and the loss rows do not move at all; the checker reports 199 of the row's 200 real classes."""
    row, rep, out, agg_ok, l2 = seeded("softmax*1.03")
    assert rep[out].bad > 100 and rep[out].row == row and rep["lse"].bad == 0 and rep["loss"].bad == 0
    assert agg_ok and l2 < 4e-3


def test_onehot_one_column_off_in_one_row_is_located():
    row, rep, out, agg_ok, _ = seeded("onehot+1")
    assert rep[out].bad == 2 and (rep[out].row, rep[out].col) == (row, 31) and f"row {row} " in rep[out].first
    assert not agg_ok                                       # a whole one-hot moved: 1 / sqrt(150) of the gradient's norm


def test_neighbours_lse_in_one_row_is_located_and_the_aggregate_misses_it():
    """Row 6 of the Gaussian case reads row 7's lse in pass 2 (1.16 larger): its loss is right (the merge was), its softmax
    part is 3.2 times too small in all 300 classes, and the aggregate's gradient rel_l2 reads 3.7e-3, under its limit of 4e-3
    (other rows of this case give 2.4e-3 ... 6.7e-2: whether the aggregate notices depends on the row)."""
    row, rep, out, agg_ok, l2 = seeded("neighbour_lse")
    assert rep[out].bad > 0 and rep[out].row == row and rep["loss"].bad == 0
    assert agg_ok and l2 < 4e-3


def test_padding_column_counted_in_psum_is_located_in_the_partial_tile():
    _, rep, out, _, _ = seeded("cols+1")
    first_valid = int(made("n512c300")[1].valid.nonzero()[0])
    assert (rep["psum"].row, rep["psum"].col) == (first_valid, 1) and rep["pmax"].bad > 0 and rep["lse"].bad > 0
    assert "column tile 1" in rep["psum"].first


def test_dropped_second_tile_of_a_lane_is_located():
    row, rep, out, agg_ok, _ = seeded("drop")
    assert rep["lse"].bad == 1 and rep["lse"].row == row and rep["loss"].row == row and rep["grad"].row == row
    assert rep["psum"].bad == 0 and rep["pmax"].bad == 0     # pass 1 was right: the merge is where it went wrong


def test_missing_rescale_when_a_later_tile_holds_the_maximum_is_located():
    row, rep, out, agg_ok, _ = seeded("norescale")
    assert rep["lse"].bad == 1 and rep["lse"].row == row and "sharp32@second" in rep["lse"].first


def test_weight0_row_leaking_0_times_exp_of_an_infinite_logit_is_located():
    row, rep, out, _, _ = seeded("0*exp(inf)")
    assert rep["grad"].row == row and rep["grad"].bad == 200 and "weight0" in rep["grad"].first


def test_missing_64_row_half_of_a_colpart_row_is_located():
    _, rep, out, agg_ok, _ = seeded("colpart-64")
    assert rep["colpart"].bad > 0 and rep["colpart"].row == 0 and rep["dbias"].bad == 0 and rep["grad"].bad == 0
    assert agg_ok                                           # (the aggregate's own column-sum line sees it: not part of this claim)


def test_cross_tile_tie_counted_as_not_top1_is_caught():
    _, rep, out, agg_ok, _ = seeded("tie_not_top1")
    assert rep["top1"].bad == 1 and "tie-inclusive" in rep["top1"].first
    assert all(v.bad == 0 for k, v in rep.items() if k != "top1") and agg_ok


def test_merge_restatement_against_fp64_on_synthetic_pairs():
    """merge_rows on the pairs the device test uses, (-inf, 0) pairs included, inside merge_reference's allowance; a (-inf, 0)
    pair as a lane's FIRST tile must not poison the lane (exp(-inf - -inf) is NaN: the pair is skipped, not multiplied by 0)."""
    for nt in R.MERGE_NTILES:
        pm, ps = R.merge_pairs(nt)
        lse, dl = R.merge_reference(pm, ps)
        got = R.merge_rows(pm, ps).double()
        frac = ((got - lse).abs() / dl)
        assert bool(torch.isfinite(got).all()) and float(frac.max()) <= 1.0, (nt, float(frac.max()))
        print(f"token-ce merge ntiles {nt}: lse model {float(frac.max()):.4f}")
