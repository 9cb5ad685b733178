"""The evaluation-row kernels at kernel level (-m gpu; csrc/eval_rows.hip), launched through the C ABI on synthetic logits as
tests/test_gpu_rowops.py launches ce_kernel, and held to tests/masked_report_ref.py (which tests/test_masked_report_host.py
holds to torch):
 * masked_report_rows: pred / rank / top-k ids exactly, logits_out and w * nll bit for bit (the latter against ce_kernel's own
   loss rows on the same inputs), nll and the log-probabilities against float64;
 * masked_report_samples: counts exactly, the per-sample mean within the fp32 summation bound, three runs bit-identical;
 * token_top1: counts exactly, ties counted, rows of weight 0 never.
Bounds. nll and a log-probability are fp32 evaluations of max + log(sum) - z: a few roundings of operands of magnitude |lse|
and |z|, the tolerance model test_gpu_rowops.py states for ce_kernel's loss rows (1e-6 of |lse| + |z| + 1, plus 1e-6 of the
value). sample_loss: masked_report_ref.sample_loss_bound (depth x ulp of the absolute row sum, as test_sum_rows)."""
import numpy as np
import pytest
import torch

from gpu_util import stream
import masked_report_ref as ref
from plbert_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 3
I_SENT, F_SENT = -77, 7.0


def _case(V, n, seed):
    g = np.random.default_rng(seed)
    z = g.uniform(-80, 80, size=(n, V)).astype(np.float32)      # exp underflows after the max shift
    z[1::3] = g.normal(0, 2, size=z[1::3].shape).astype(np.float32)
    tgt = g.integers(0, V, size=n).astype(np.int32)
    z[0] = 3.0                                                   # equal logits: pred 0, rank = the label
    tgt[0] = V - 1
    if n > 1:
        tgt[1] = 0
    if n > 2:                                                    # the label ties the maximum at a higher index: rank 1
        z[2] = g.normal(0, 1, size=V).astype(np.float32)
        z[2, 1] = z[2, V - 1] = 9.0
        tgt[2] = V - 1
    if n > 3:
        z[3, int(g.integers(0, V))] = np.nan                     # one NaN row
    if n > 7:
        z[7] = g.integers(0, 3, size=V).astype(np.float32)      # few distinct values: ties everywhere
    return z, tgt


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _launch_rows(z, tgt, V, topk, ldl):
    L = _lib.lib()
    n = z.shape[0]
    src = np.full((n, ldl), 1e4, np.float32)                     # columns >= V must not count
    src[:, :V] = z
    d_src, d_tgt = _dev(src), _dev(tgt)
    rows = n + GUARD
    out = {"pred": torch.full((rows,), I_SENT, dtype=torch.int32, device=DEV),
           "rank": torch.full((rows,), I_SENT, dtype=torch.int32, device=DEV),
           "nll": torch.full((rows,), F_SENT, device=DEV),
           "ids": torch.full((rows, max(topk, 1)), I_SENT, dtype=torch.int32, device=DEV),
           "lp": torch.full((rows, max(topk, 1)), F_SENT, device=DEV),
           "logits": torch.full((rows, V), F_SENT, device=DEV)}
    assert L.plb_launch_masked_report_rows(d_src.data_ptr(), ldl, V, d_tgt.data_ptr(), n, topk, out["pred"].data_ptr(),
                                           out["rank"].data_ptr(), out["nll"].data_ptr(), out["ids"].data_ptr(),
                                           out["lp"].data_ptr(), out["logits"].data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    return d_src, d_tgt, {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("n", [1, 3, 4, 5, 129])
@pytest.mark.parametrize("V", [4, 12, 188, 256])
def test_rows_against_the_instrument(V, n):
    L = _lib.lib()
    z, tgt = _case(V, n, seed=1000 * V + n)
    ldl = V + 5
    zd = z.astype(np.float64)
    for topk in (0, 1, 5, 8):
        d_src, d_tgt, got = _launch_rows(z, tgt, V, topk, ldl)
        want = ref.rows(z, tgt, topk)
        ok = ~want.nan
        assert np.array_equal(got["pred"][:n], want.pred) and np.array_equal(got["rank"][:n], want.rank), topk
        assert np.array_equal(got["logits"][:n].view(np.uint32), z.view(np.uint32))          # a copy, NaN payload included
        if topk:
            assert np.array_equal(got["ids"][:n, :topk], want.topk_ids), topk
            lp, wlp = got["lp"][:n, :topk].astype(np.float64), want.topk_logprob
            assert np.isnan(lp[~ok]).all() and np.array_equal(np.isneginf(lp[ok]), np.isneginf(wlp[ok]))   # tail past V: -inf
            fin = np.isfinite(wlp) & ok[:, None]
            zsel = np.take_along_axis(zd, np.clip(want.topk_ids, 0, V - 1).astype(np.int64), 1)
            tol = 1e-6 * np.abs(wlp) + 1e-6 * (np.abs(want.lse)[:, None] + np.abs(zsel) + 1)
            err = np.abs(np.where(fin, lp, 0.0) - np.where(fin, wlp, 0.0))
            assert bool((err[fin] <= tol[fin]).all()), float((err[fin] / tol[fin]).max())
        zt = zd[np.arange(n), tgt]
        nll = got["nll"][:n].astype(np.float64)
        assert np.isnan(nll[~ok]).all()
        tol = 1e-6 * np.abs(want.nll) + 1e-6 * (np.abs(want.lse) + np.abs(zt) + 1)
        assert bool((np.abs(nll - want.nll)[ok] <= tol[ok]).all()), float((np.abs(nll - want.nll)[ok] / tol[ok]).max())
        # the guard rows behind n stay untouched
        for k, sent in (("pred", I_SENT), ("rank", I_SENT), ("ids", I_SENT), ("nll", F_SENT), ("lp", F_SENT), ("logits", F_SENT)):
            assert bool((got[k][n:] == sent).all()), (k, topk)
        if not topk:
            assert bool((got["ids"] == I_SENT).all()) and bool((got["lp"] == F_SENT).all())
    # the invariants, on the kernel's own outputs
    assert np.array_equal(got["pred"][:n] == tgt, got["rank"][:n] == 0)
    assert got["pred"][0] == 0 and got["rank"][0] == V - 1
    if n > 2:
        assert got["rank"][2] == 1 and got["pred"][2] == 1
    if n > 3:
        assert got["pred"][3] == -1 and got["rank"][3] == V and bool((got["ids"][3] == -1).all())
    # w * nll is ce_kernel's loss row, bit for bit
    npad = n + GUARD
    w = (1.0 / np.random.default_rng(n).integers(1, 50, size=n)).astype(np.float32)
    d_w = _dev(w)
    loss_rows = torch.full((npad,), F_SENT, device=DEV)
    dlog = torch.zeros((npad, 256), dtype=torch.bfloat16, device=DEV)
    assert L.plb_launch_ce_fwd_bwd(d_src.data_ptr(), ldl, V, d_tgt.data_ptr(), d_w.data_ptr(), n, npad, loss_rows.data_ptr(),
                                   dlog.data_ptr(), 256, stream()) == 0
    torch.cuda.synchronize()
    ce = loss_rows.cpu().numpy()[:n]
    mine = w * got["nll"][:n]                                                                # one fp32 multiply, as the kernel's
    assert np.isnan(ce[~ok]).all() and np.isnan(mine[~ok]).all()
    assert np.array_equal(ce[ok].view(np.uint32), mine[ok].view(np.uint32))


def test_rows_with_only_some_outputs():
    """Every output pointer is optional: pred alone, the list alone, nothing but the copy."""
    L = _lib.lib()
    V, n = 188, 6
    z, tgt = _case(V, n, seed=3)
    want = ref.rows(z, tgt, 5)
    d_src, d_tgt = _dev(z), _dev(tgt)
    pred = torch.full((n,), I_SENT, dtype=torch.int32, device=DEV)
    ids = torch.full((n, 5), I_SENT, dtype=torch.int32, device=DEV)
    copy = torch.full((n, V), F_SENT, device=DEV)
    for args in ((pred.data_ptr(), None, None, None, None, None), (None, None, None, ids.data_ptr(), None, None),
                 (None, None, None, None, None, copy.data_ptr())):
        assert L.plb_launch_masked_report_rows(d_src.data_ptr(), V, V, d_tgt.data_ptr(), n, 5, *args, stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(pred.cpu().numpy(), want.pred) and np.array_equal(ids.cpu().numpy(), want.topk_ids)
    assert np.array_equal(copy.cpu().numpy().view(np.uint32), z.view(np.uint32))


def test_rows_refuses_what_it_cannot_run():
    L = _lib.lib()
    buf = torch.zeros(4096, device=DEV)
    p = buf.data_ptr()
    for V, topk in ((257, 5), (10, 5), (188, 9), (188, -1), (0, 1)):
        assert L.plb_launch_masked_report_rows(p, 300, V, p, 1, topk, p, p, p, p, p, p, stream()) != 0, (V, topk)
    assert L.plb_launch_masked_report_rows(p, 100, 188, p, 1, 5, p, p, p, p, p, p, stream()) != 0       # ldl < V
    assert L.plb_launch_masked_report_samples(p, 1025, p, p, 5, p, p, p, p, stream()) != 0
    assert L.plb_launch_masked_report_samples(p, 4, p, p, 9, p, p, p, p, stream()) != 0
    assert L.plb_launch_token_top1(p, 0, p, p, 4, p, p, stream()) != 0
    torch.cuda.synchronize()
    assert bool((buf == 0).all())                                                                       # nothing was launched


@pytest.mark.parametrize("counts", [[300], [5, 0, 17, 1, 0, 40], [0, 0, 0, 0, 0, 0], [77, 76, 0, 80, 12, 64, 0, 3]])
def test_samples(counts):
    L = _lib.lib()
    B, n = len(counts), sum(counts)
    g = np.random.default_rng(n + B)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rank = g.integers(0, 9, size=max(n, 1)).astype(np.int32)
    nll = g.uniform(0, 12, size=max(n, 1)).astype(np.float32)
    d_off, d_rank, d_nll = _dev(off), _dev(rank), _dev(nll)
    for topk in (5, 0):
        runs = []
        for _ in range(3):
            loss = torch.full((B + GUARD,), F_SENT, device=DEV)
            top1 = torch.full((B + GUARD,), I_SENT, dtype=torch.int32, device=DEV)
            tk = torch.full((B + GUARD,), I_SENT, dtype=torch.int32, device=DEV)
            tot = torch.full((4 + GUARD,), I_SENT, dtype=torch.int32, device=DEV)
            assert L.plb_launch_masked_report_samples(d_off.data_ptr(), B, d_rank.data_ptr(), d_nll.data_ptr(), topk,
                                                      loss.data_ptr(), top1.data_ptr(), tk.data_ptr(), tot.data_ptr(),
                                                      stream()) == 0
            torch.cuda.synchronize()
            runs.append([t.cpu().numpy() for t in (loss, top1, tk, tot)])
        for r in runs[1:]:
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(r, runs[0]))
        loss, top1, tk, tot = runs[0]
        want = ref.samples(off, rank[:n], nll[:n], topk)
        assert np.array_equal(top1[:B], want.top1) and np.array_equal(tk[:B], want.topk) and np.array_equal(tot[:4], want.totals)
        err, bound = np.abs(loss[:B].astype(np.float64) - want.loss), ref.sample_loss_bound(off, nll[:n])
        assert bool((err <= bound).all()), (err, bound)
        assert bool((loss[:B][np.diff(off) == 0] == 0).all())                                 # a sample without rows: exactly 0
        assert bool((loss[B:] == F_SENT).all()) and all(bool((t[m:] == I_SENT).all()) for t, m in ((top1, B), (tk, B), (tot, 4)))
    # totals alone (one launch), sample outputs alone
    tot = torch.full((4,), I_SENT, dtype=torch.int32, device=DEV)
    top1 = torch.full((B,), I_SENT, dtype=torch.int32, device=DEV)
    assert L.plb_launch_masked_report_samples(d_off.data_ptr(), B, d_rank.data_ptr(), None, 5, None, None, None, tot.data_ptr(),
                                              stream()) == 0
    assert L.plb_launch_masked_report_samples(d_off.data_ptr(), B, d_rank.data_ptr(), None, 5, None, top1.data_ptr(), None, None,
                                              stream()) == 0
    torch.cuda.synchronize()
    want = ref.samples(off, rank[:n], nll[:n], 5)
    assert np.array_equal(tot.cpu().numpy(), want.totals) and np.array_equal(top1.cpu().numpy(), want.top1)


@pytest.mark.parametrize("rows", [1, 133])
@pytest.mark.parametrize("ntiles", [1, 3, 250])
def test_token_top1(ntiles, rows):
    L = _lib.lib()
    g = np.random.default_rng(ntiles * 1000 + rows)
    pmax = g.normal(0, 3, size=(rows, ntiles)).astype(np.float32)
    pmax[g.random(size=(rows, ntiles)) < 0.1] = -np.inf                   # a tile whose columns are all padding
    pmax[:, 0] = np.where(np.isneginf(pmax).all(1), 0.5, pmax[:, 0])
    mx = pmax.max(1)
    tl = (mx - g.uniform(0.1, 5, size=rows)).astype(np.float32)           # wrong by default
    kind = g.integers(0, 4, size=rows)                                    # 0 wrong, 1 correct, 2 correct with a tie, 3 weight 0
    kind[0] = 1
    tl[kind >= 1] = mx[kind >= 1]
    if ntiles > 1:
        for r in np.nonzero(kind == 2)[0]:                                # another tile holds the same maximum
            pmax[r, (int(pmax[r].argmax()) + 1) % ntiles] = mx[r]
    w = np.where(kind == 3, 0.0, 1.0 / 77).astype(np.float32)             # weight 0 rows carry the "correct" pattern
    d_p, d_t, d_w = _dev(pmax), _dev(tl), _dev(w)
    nb = (rows + 3) // 4
    outs = []
    for _ in range(3):
        scratch = torch.full((2 * nb + GUARD,), I_SENT, dtype=torch.int32, device=DEV)
        tot = torch.full((2 + GUARD,), I_SENT, dtype=torch.int32, device=DEV)
        assert L.plb_launch_token_top1(d_p.data_ptr(), ntiles, d_t.data_ptr(), d_w.data_ptr(), rows, scratch.data_ptr(),
                                       tot.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        outs.append(tot.cpu().numpy())
        assert bool((scratch[2 * nb:] == I_SENT).all())
    want = ref.token_top1(pmax, tl, w)
    assert want.tolist() == [int((kind != 3).sum()), int(((kind == 1) | (kind == 2)).sum())]
    assert all(np.array_equal(o[:2], want) and bool((o[2:] == I_SENT).all()) for o in outs)
