"""The instrument of tests/test_gpu_layernorm_rows.py, proved on the CPU before a GPU sees it (not marked gpu):
 * honest fp32 arithmetic — a numpy float32 LayerNorm forward and backward that follows the kernels' formulas, rounded to
   bf16 — passes check_ln_elements at DELTA0 and the partial-sum bound on every class, using at most HALF of the fp32
   allowance (if a class needs more, the class or the condition term is wrong, not a kernel);
 * the checker names row and column of five simulated defects, each of which leaves rel_l2 of the whole matrix below the
   3e-3 ... 5e-3 thresholds of the aggregate tests;
 * the tile restatement reproduces the conditioning of form 5 (one-pass variance per tile) measured on the CPU: relative
   rstd error 1.7e-6 / 9e-7 at mean / std = 4 and 2.2e-5 / 1.2e-5 at 16 (tiles of 384 / 256), within a factor 2;
 * LN_NEARCONST_SEED yields near-constant rows whose merged M2 is <= 0 in that restatement: the rows that need the clamp in
   csrc/gemm_nt_pipeline.h."""
import numpy as np
import pytest
import torch

from gpu_util import (DELTA0, LN_BWD_CLASSES, LN_CLASSES, LN_NEARCONST_SEED, LN_STAT_FLOOR, check_ln_elements, check_ln_partials,
                      check_ln_stats, lane_tree_sum, layernorm_bwd_fp64, layernorm_fp64, layernorm_stats_f32,
                      ln_class_worst, ln_dy, ln_fwd_cond, ln_row_bound, ln_rows, rel_l2)

f32 = np.float32


def _affine(H, seed):
    g = torch.Generator().manual_seed(seed)
    return 1.0 + 0.3 * torch.randn(H, generator=g), 0.2 * torch.randn(H, generator=g)


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16)


def forward_f32(x, gamma, beta):
    """The standalone forward in float32 numpy: statistics of the two-pass restatement (order 0), then
    (x - mean) * rstd * gamma + beta as the kernels write it, stored as bf16."""
    st = layernorm_stats_f32(x, "two_pass", orders=1)
    v = x.float().numpy()
    y = (v - st.mean[:, None]) * st.rstd[:, None] * gamma.numpy() + beta.numpy()
    assert y.dtype == np.float32
    return _bf16(y), torch.from_numpy(st.mean), torch.from_numpy(st.rstd)


def backward_f32(x, mean, rstd, gamma, dy):
    """The standalone backward in float32 numpy (csrc/layernorm.hip ln_bwd_kernel): one lane set walks every row, so each
    column sum is a chain of T additions."""
    v, d, g = x.float().numpy(), dy.float().numpy(), gamma.numpy()
    H = v.shape[1]
    inv = f32(1.0) / f32(H)
    xh = (v - mean.numpy()[:, None]) * rstd.numpy()[:, None]
    dxh = d * g
    s1 = (lane_tree_sum(dxh) * inv)[:, None]
    s2 = (lane_tree_sum(dxh * xh) * inv)[:, None]
    dx = _bf16(rstd.numpy()[:, None] * (dxh - s1 - xh * s2))
    dg, db, cs = np.zeros(H, f32), np.zeros(H, f32), np.zeros(H, f32)
    stored = dx.float().numpy()
    for t in range(v.shape[0]):
        dg = dg + d[t] * xh[t]
        db = db + d[t]
        cs = cs + stored[t]
    return dx, torch.from_numpy(dg), torch.from_numpy(db), torch.from_numpy(cs)


def _fwd_case(H, T=72, seed=1):
    x, cls = ln_rows(T, H, seed)
    gamma, beta = _affine(H, seed + 1)
    mean, rstd, xhat, y = layernorm_fp64(x, gamma, beta)
    return x, cls, gamma, beta, (mean, rstd, xhat, y)


def _bwd_case(H, T=72, seed=2):
    x, cls = ln_rows(T, H, seed, LN_BWD_CLASSES)
    gamma, _ = _affine(H, seed + 1)
    dy, kind = ln_dy(T, H, seed + 2)
    m64, r64, _, _ = layernorm_fp64(x, gamma, torch.zeros(H))
    mean, rstd = m64.float(), r64.float()
    return x, cls, gamma, dy, kind, mean, rstd, layernorm_bwd_fp64(x, mean, rstd, gamma, dy)


@pytest.mark.parametrize("H", [4, 132, 768, 1024])
def test_honest_fp32_forward_uses_half_the_allowance(H):
    x, cls, gamma, beta, (mean, rstd, xhat, y) = _fwd_case(H)
    got, m32, r32 = forward_f32(x, gamma, beta)
    shares = check_ln_elements(f"fp32 forward H {H}", got, y, ln_fwd_cond(xhat, gamma, beta, mean, rstd), DELTA0, cls)
    print(f"ln host forward H {H}: y " + " ".join(f"{k} {v:.2f}" for k, v in shares.items()))
    assert max(shares.values()) <= 0.5, shares
    st = layernorm_stats_f32(x, "two_pass")
    bm = ln_row_bound(ln_class_worst(st.mean_err, cls, LN_CLASSES), cls, LN_CLASSES, LN_STAT_FLOOR)
    br = ln_row_bound(ln_class_worst(st.rstd_err, cls, LN_CLASSES), cls, LN_CLASSES, LN_STAT_FLOOR)
    em, es = check_ln_stats(f"fp32 forward H {H}", m32, r32, x, bm, br, cls)
    assert float(em.max()) <= 0.5 * float(bm.min()) and float(es.max()) <= 0.5 * float(br.min()), (em.max(), es.max())
    zero = cls == LN_CLASSES.index("zero")
    assert torch.equal(got[zero], beta.to(torch.bfloat16).expand(int(zero.sum()), H))       # y == bf16(beta) exactly
    assert bool(((r32[zero].double() * 1e-6 - 1.0).abs() <= LN_STAT_FLOOR).all())            # rstd = eps^-1/2


@pytest.mark.parametrize("H", [4, 132, 768, 1024])
def test_honest_fp32_backward_uses_half_the_allowance(H):
    x, cls, gamma, dy, kind, mean, rstd, ref = _bwd_case(H)
    dx, dg, db, cs = backward_f32(x, mean, rstd, gamma, dy)
    shares = check_ln_elements(f"fp32 backward H {H}", dx, ref.dx, ref.cond, DELTA0, cls, LN_BWD_CLASSES)
    print(f"ln host backward H {H}: dx " + " ".join(f"{k} {v:.2f}" for k, v in shares.items()))
    assert max(shares.values()) <= 0.5, shares
    assert bool((dx[kind == 3] == 0).all())                                                # an all-zero dy row: dx exactly zero
    T = x.shape[0]
    stored = dx.double()
    for what, got, want, mag in (("dgamma", dg, ref.dgamma, ref.mag_gamma), ("dbeta", db, ref.dbeta, ref.mag_beta),
                                 ("colsum", cs, stored.sum(0), stored.abs().sum(0))):
        ratio = check_ln_partials(f"fp32 backward H {H} {what}", got, want, mag, T)
        print(f"ln host backward H {H}: {what} {ratio:.2f}")
        assert ratio <= 0.5, (what, ratio)


def _raises_at(row, col, fn):
    with pytest.raises(AssertionError) as e:
        fn()
    assert f"element ({row}, {col})" in str(e.value), str(e.value)


def test_checker_locates_simulated_defects():
    H, T = 768, 1153                                                 # odd T; 128 rows of every class
    x, cls, gamma, beta, (mean, rstd, xhat, y) = _fwd_case(H, T)
    good, _, _ = forward_f32(x, gamma, beta)
    cond = ln_fwd_cond(xhat, gamma, beta, mean, rstd)
    check = lambda got: check_ln_elements("forward", got, y, cond, DELTA0, cls)   # noqa: E731
    check(good)
    # one element computed with its neighbour's gamma (row 9: class plain; a column where that moves y by about 0.1)
    r = 9
    c = int((((gamma[1:] - gamma[:-1]).double() * xhat[r, :-1]).abs() - 0.1).abs().argmin())
    bad = good.clone()
    bad[r, c] = (xhat[r, c] * gamma[c + 1].double() + beta[c].double()).to(torch.bfloat16)
    assert rel_l2(bad.float(), y) < 3e-3
    _raises_at(r, c, lambda: check(bad))
    # one row normalised with the next row's statistics (rows 0 and 9 are both N(0,1): the aggregate does not move)
    bad = good.clone()
    m2, r2 = mean[9], rstd[9]
    bad[0] = (((x[0].double() - m2) * r2) * gamma.double() + beta.double()).to(torch.bfloat16)
    assert rel_l2(bad.float(), y) < 3e-3
    with pytest.raises(AssertionError, match=r"element \(0, \d+\) of class plain"):
        check(bad)
    # one element off by exactly one bf16 spacing, away from the reference
    r, c = 27, 300
    bad = good.clone()
    step = 1 if (good[r, c].double() >= y[r, c]) == (good[r, c] >= 0) else -1          # one step further from y
    bad.view(torch.int16)[r, c] += step
    assert rel_l2(bad.float(), y) < 3e-3
    _raises_at(r, c, lambda: check(bad))
    # backward
    x, cls, gamma, dy, kind, mean, rstd, ref = _bwd_case(H, T)
    dx, dg, db, cs = backward_f32(x, mean, rstd, gamma, dy)
    check_ln_elements("backward", dx, ref.dx, ref.cond, DELTA0, cls, LN_BWD_CLASSES)
    # the last row of an odd T dropped from dbeta (its dy is N(0,1) here)
    assert int(kind[T - 1]) != 3
    short = db - dy[T - 1].float()
    assert rel_l2(short, ref.dbeta) > 0 and rel_l2(torch.cat([dg, short]), torch.cat([ref.dgamma, ref.dbeta])) < 0.2
    with pytest.raises(AssertionError, match=r"dbeta: column \d+"):
        check_ln_partials("dbeta", short, ref.dbeta, ref.mag_beta, T)
    # a dx row whose s2 term was left out (row 24: class plain, dy N(0,1): s2 ~ N(0, 1/H) — the row moves by ~ 4e-2 of its
    # norm, the matrix by 4e-2 / sqrt(T))
    r = 24
    assert int(cls[r]) == 0 and int(kind[r]) == 0
    g64 = dy[r].double() * gamma.double()
    bad = dx.clone()
    bad[r] = (rstd[r].double() * (g64 - g64.mean())).to(torch.bfloat16)
    assert rel_l2(bad.float(), ref.dx) < 5e-3
    with pytest.raises(AssertionError, match=rf"element \({r}, \d+\) of class plain"):
        check_ln_elements("backward", bad, ref.dx, ref.cond, DELTA0, cls, LN_BWD_CLASSES)


@pytest.mark.parametrize("ratio,cname,want", [(4, "off4", (1.7e-6, 9e-7)), (16, "off16", (2.2e-5, 1.2e-5))])
def test_tile_restatement_reproduces_the_conditioning_of_form_5(ratio, cname, want):
    for (N, TN), w in zip(((768, 384), (1024, 256)), want):
        x, _ = ln_rows(512, N, 5, (cname,))
        tile = float(layernorm_stats_f32(x, ("tile", TN)).rstd_err.max())
        two = float(layernorm_stats_f32(x, "two_pass").rstd_err.max())
        print(f"ln host conditioning: mean/std {ratio} tile {TN}: one pass {tile:.2e} two pass {two:.2e}")
        assert w / 2 <= tile <= 2 * w, (ratio, TN, tile, w)
        assert two <= 3e-7, two                                      # the standalone form does not see the offset


def test_committed_seed_yields_a_nonpositive_m2():
    x, _ = ln_rows(1024, 768, LN_NEARCONST_SEED, ("nearconst",))
    st = layernorm_stats_f32(x, ("tile", 384))
    n = int((st.m2 <= 0).sum())
    print(f"ln host nearconst: {n} of 1024 rows with m2 <= 0 at tile 384, smallest {st.m2.min():.3e}")
    assert n >= 1
    assert np.isfinite(st.rstd).all() and (st.rstd > 0).all()        # the restatement clamps, as the kernel does
    two = layernorm_stats_f32(x, "two_pass")
    assert float(two.rstd_err.max()) <= 4 * LN_STAT_FLOOR             # the standalone kernels are well-conditioned there
