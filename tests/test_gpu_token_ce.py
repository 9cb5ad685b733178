"""-m gpu: the fused token-head cross-entropy per element (plb_launch_gemm_nt_big act 3 -> plb_launch_token_ce_combine[_packed]
-> act 4 -> plb_launch_colsum, with plb_launch_sum_rows and plb_launch_token_top1 on the same outputs), on both tile forms
the engine picks between (256x256 and 128x256), against token_ce_ref's float64 reference under the allowances derived in that
module's docstring. The operands give logits that are exact fp32 numbers (integer multiples of 2^-4, the premise asserted
before every launch), so pass 1's maxima and target logits are held bit for bit and everything else only has to pay for the
exponential, the logarithm, the merges and one bf16 rounding. What the rows hold — soft, sharp (gap 32 / 80 / 128 with the
winner in tile 0, in the last real class, in a lane's second, last and first merge iteration), offset (+80, and -80 through
the bias), exact ties across and inside tiles, targets on tile and strip edges, rows of weight 0 with +-inf / NaN / 3e38 hidden
states and the targets -1, ce_cols, N + 5, 2^40 — is described there; the class of a row is in every failure message.
tests/test_token_ce_host.py proves the instrument on the CPU (the restatement inside every allowance, nine seeded defects
caught and located, the ones the former aggregate misses named).

Largest fraction of each allowance used by the CPU restatement (`model`; the same for both forms except colpart / dbias,
where the 1256 form's is given), per case, from tests/test_token_ce_host.py -s:
    case            psum     lse      loss     grad     colpart  dbias
    n256c200        0.0052   0.1439   0.0870   0.4962   0.0000   0.0000
    n512c300        0.0033   0.0955   0.0935   0.4950   0.0000   0.0000
    n512c512        0.0063   0.1349   0.0942   0.4971   0.0000   0.0000
    n16640c16500    0.0075   0.1283   0.0797   0.4955   0.0115   0.0079
    n64000c64000    0.0098   0.1647   0.0992   0.4895   0.0287   0.0117
    packed          0.0033   0.0955   0.0827   0.4954   0.0000   0.0000
    gauss           0.0004   0.0005   0.0005   0.4998   0.0763   0.0110
pmax, tlogit, w, the required zeros and the top-1 totals are exact (fraction 0). The allowances are the derived ones; none
was calibrated on the restatement (the 4 x rule was not needed: every constant comes from the code or from the ISA's 1 ulp
for V_EXP_F32 / V_LOG_F32), so the model sits far inside psum's 256 u, which is a worst-case chain bound.
Largest fraction of each allowance used by the KERNELS, first run on an MI355X (pytest -s prints `token-ce <case> form <f>:
<output> model <fraction> kernel <fraction> at <element>`); pmax, tlogit, w and top1 read 0 on every exact case:
    case / form          psum     lse      loss     grad     colpart  dbias    loss_sum
    n256c200      256    0.0052   0.1439   0.0870   0.4962   0.0000   0.0000   0.0016
    n256c200      1256   0.0052   0.1439   0.0870   0.4962   0.0000   0.0000   0.0016
    n512c300      256    0.0037   0.0955   0.0935   0.4950   0.0000   0.0000   0.0162
    n512c300      1256   0.0037   0.0955   0.0935   0.4950   0.0000   0.0000   0.0162
    n512c512      256    0.0044   0.1349   0.0942   0.4971   0.0000   0.0000   0.0954
    n512c512      1256   0.0044   0.1349   0.0942   0.4971   0.0000   0.0000   0.0954
    n16640c16500  256    0.0098   0.1764   0.1105   0.4955   0.0029   0.0044   0.0603
    n16640c16500  1256   0.0098   0.1764   0.1105   0.4955   0.0115   0.0138   0.0603
    n64000c64000  256    0.0093   0.1647   0.0992   0.4895   0.0217   0.0197   0.0449
    n64000c64000  1256   0.0093   0.1647   0.0992   0.4895   0.0239   0.0197   0.0449
    packed        256    0.0037   0.0955   0.0827   0.4954   0.0000   0.0000   0.0635
    packed        1256   0.0037   0.0955   0.0827   0.4954   0.0000   0.0000   0.0635
    gauss         256    0.0003   0.0002   0.0003   0.4998   0.0264   0.0228   0.1393   (pmax 0.0014, tlogit 0.0007 of dz)
    gauss         1256   0.0003   0.0002   0.0003   0.4998   0.0487   0.0404   0.1393   (pmax 0.0012, tlogit 0.0005 of dz)
    merge alone, ntiles 1 / 4 / 64 / 65 / 250: lse 0.0901 / 0.4071 / 0.3692 / 0.3735 / 0.3567 (model 0.1416, then the same)
No fraction is above 1 and none is above 1.4 x the restatement's: the device's exp / log behave as the model's here.
One defect was found, by reading token_ce_merge_row for the (-inf, 0) case: as a lane's FIRST tile such a pair made
l = 0 * exp(-inf - -inf) = NaN for the rest of the lane (ntiles > 64 with a padding tile in 0..63; the engine pads N by less
than a tile, so no engine call reached it). The pair is now skipped; test_merge_kernels_on_synthetic_pairs[65] and [250]
hold it.
"""
import pytest
import torch

import token_ce_ref as R
from gpu_util import EXACT_LIMIT, stream
from plbert_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def report(name, form, rep):
    model = R.modelled(name, R.FORMS[form])
    for out, v in rep.items():
        print(f"token-ce {name} form {form}: {out} model {model[out].frac:.4f} kernel {v.frac:.4f} at {v.at}")


@pytest.mark.parametrize("form", list(R.FORMS))
@pytest.mark.parametrize("name", list(R.CASES))
def test_every_output_element_against_fp64(name, form):
    """The whole chain, twice: every output inside its allowance (check() compares per element and names the first offender
    with its row class), the runs bit-identical, the underflow count as designed; on the packed case the padded merge over the
    same pass-1 output gives the same bits."""
    case, ops, ref, allow = R.made(name)
    if case.exact:
        assert R.premise(ops) < EXACT_LIMIT
    assert R.floor_count(ref) == ops.floor_designed
    got = R.launch(ops, case, form)
    rep = R.check(got, ref, allow, ops.cls, case.exact)
    report(name, form, rep)
    assert not R.failures(rep), "\n".join(R.failures(rep))
    # rows of weight 0: nothing of their infinite / NaN hidden states anywhere (check() holds their zeros; NaN would fail every sum)
    assert bool(torch.isfinite(got.colpart).all()) and bool(torch.isfinite(got.dbias).all())
    assert bool(torch.isfinite(got.grad.float()).all()) and bool((got.grad[~ref.valid] == 0).all())
    assert bool((got.grad[:, case.ce_cols:] == 0).all()) and bool((got.colpart[:, case.ce_cols:] == 0).all())
    # ce_tlogit of a row of weight 0 whose target names no column keeps its prefill (a target in [0, N) after the
    # conversion to int may have it written: it is never read — lse, w and the loss row above are exact zeros)
    unnamed = (~ref.valid) & ((ops.tgt == -1) | (ops.tgt == case.N + 5))
    assert int(unnamed.sum()) > 0 and bool(torch.isnan(got.tlogit[unnamed]).all())
    again = R.launch(ops, case, form)
    assert R.same_bits(got, again) == []
    if case.row_start is not None:
        padded = R.launch(ops, case, form, packed_merge=False)
        assert R.same_bits(got, padded) == []


def _merge(pm, ps, packed):
    L = _lib.lib()
    rows, nt = pm.shape
    nan = float("nan")
    pmd, psd = pm.to(DEV), ps.to(DEV)
    tl = torch.zeros(rows, device=DEV)
    lse, w, loss = (torch.full((rows + 3,), nan, device=DEV) for _ in range(3))
    lengths = torch.tensor([rows], dtype=torch.int32, device=DEV)
    plan = torch.tensor([0, rows], dtype=torch.int32, device=DEV)
    if packed:
        assert L.plb_launch_token_ce_combine_packed(pmd.data_ptr(), psd.data_ptr(), nt, tl.data_ptr(), lengths.data_ptr(),
                                                    plan.data_ptr(), 1, rows, rows, lse.data_ptr(), w.data_ptr(), loss.data_ptr(),
                                                    stream()) == 0
    else:
        assert L.plb_launch_token_ce_combine(pmd.data_ptr(), psd.data_ptr(), nt, tl.data_ptr(), lengths.data_ptr(), 1, rows, rows,
                                             lse.data_ptr(), w.data_ptr(), loss.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t[rows:]).all()) for t in (lse, w, loss))          # nothing written behind `rows`
    return lse[:rows].cpu(), w[:rows].cpu(), loss[:rows].cpu()


@pytest.mark.parametrize("nt", R.MERGE_NTILES)
def test_merge_kernels_on_synthetic_pairs(nt):
    """The two merge kernels alone against the float64 log-sum-exp of the pairs: ntiles 1 / 4 / 64 / 65 / 250 (lanes with no,
    one, two, three and four tiles), maxima over +-80 ascending, descending and shuffled within a lane (the rescale taken on
    every iteration, on none, on some), a (-inf, 0) pair — a tile without a real class, which pass 1 produces when N is
    padded by a whole tile — as a lane's first tile and as a later one. The packed kernel gives the padded kernel's bits."""
    pm, ps = R.merge_pairs(nt)
    want, dl = R.merge_reference(pm, ps)
    lse, w, loss = _merge(pm, ps, packed=False)
    frac = (lse.double() - want).abs() / dl
    frac = torch.where(torch.isnan(frac), torch.full_like(frac, float("inf")), frac)
    i = int(frac.argmax())
    model = float(((R.merge_rows(pm, ps).double() - want).abs() / dl).max())
    print(f"token-ce merge ntiles {nt}: lse model {model:.4f} kernel {float(frac[i]):.4f} at row {i}: got {float(lse[i])!r}, want {float(want[i])!r}")
    bad = (frac > 1.0).nonzero().flatten().tolist()
    assert not bad, f"{len(bad)} of {len(frac)} rows outside; first row {bad[0]}: got {float(lse[bad[0]])!r}, want {float(want[bad[0]])!r}"
    rows = pm.shape[0]
    assert torch.equal(w, torch.full((rows,), 1.0) / float(rows))
    wl = w.double() * want
    assert bool(((loss.double() - wl).abs() <= w.double() * (dl + 2.0 ** -23 * want.abs())).all())
    for a, b in zip((lse, w, loss), _merge(pm, ps, packed=True)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
