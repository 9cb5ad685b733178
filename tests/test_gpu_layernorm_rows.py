"""Per-element LayerNorm parity (-m gpu): every LayerNorm kernel form against float64, element by element, on rows of nine
value classes (gpu_util.ln_rows) and at the row tails, strides and grid shapes the aggregate tests never reach.

The contract (gpu_util.check_ln_elements): |got - ref| <= 0.5 x spacing_bf16(ref) + delta x cond per element, ref the float64
evaluation of the inputs as stored; delta = DELTA0 = 2^-18 everywhere except the forward of the fused forms, where it is
max(DELTA0, 4 x the class's worst rstd error in the float32 restatement of form 5's one-pass-per-tile variance
(gpu_util.layernorm_stats_f32)). Statistics per row: relative rstd error and |mean - mu| / (|mu| + sigma) within
max(2^-20, 4 x restated). Column sums (dgamma, dbeta, column sums of dx as stored): partial rows summed in float64, per
column within (rows_per_lane + 8) x 2^-24 x sum |term|. No bound is taken from a kernel's output.

Which instantiation a case runs follows from the launchers' conditions (csrc/layernorm.hip plb_launch_ln_fwd / _bwd; the
launch profile has one class per launcher, not per instantiation), and the case ids name it:
  forward   H = 768 / 1024 with ldx % 8 == 0 and ldy % 8 == 0 -> ln_fwd_wide_kernel<96 | 128>; else ln_fwd_kernel<ceil(H / 256)>
  backward  H = 1024 with every ld % 8 == 0, or out8 at 768 / 1024 -> ln_bwd_wide_kernel<128 | 96>; else ln_bwd_kernel<ceil(H / 256)>
  fused     N % 384 == 0 -> the 128x384 tile, else 128x256; plb_launch_gemm_nt_ln = bf16 forms 5 / 6 (csrc/gemm_ln.hip),
            plb_launch_gemm_nt_fp8_ln = fp8 forms 5 / 6 (csrc/gemm_fp8_ln.hip; form 6 there is the LEAN epilogue)

Worst relative rstd error per class of form 5 (bf16, bias 0, M = 1024) at N = 768 (two tiles of 384) / N = 1024 (four tiles of
256): the restatement (CPU, the worst of 8 summation orders, each with and without the contraction of pb - pa * mt) and the
kernel on an MI355X (the first `-s` run). The rows are the class's residual plus an integer GEMM term of standard deviation
0.8, so off4 / off16 have mean / std = 3 / 12 here.

  class      restated 768 / 1024     kernel 768 / 1024
  plain      1.3e-07 / 9.1e-08       9.7e-08 / 6.8e-08
  off4       6.5e-07 / 4.0e-07       5.1e-07 / 3.4e-07
  off16      1.0e-05 / 6.0e-06       8.3e-06 / 4.5e-06
  small      1.5e-07 / 1.2e-07       1.0e-07 / 1.1e-07
  eps        1.0e-07 / 1.1e-07       8.1e-08 / 1.1e-07
  large      1.2e-07 / 1.0e-07       8.9e-08 / 8.5e-08
  spike      2.1e-07 / 1.9e-07       1.7e-07 / 1.3e-07
  zero       0 / 0                   0 / 0
  nearconst  83 of 1024 rows with M2 <= 0 at N = 768 (none at 1024); kernel, with the clamp: every row finite, rstd <= 1e6
The fp8 form gives the same figures within 20 %. The standalone kernels (two-pass), every case: rstd restated <= 3.3e-07,
kernel <= 2.4e-07; mean restated <= 7.9e-08, kernel <= 7.9e-08. No element of any case used more than 4 % of its delta x cond;
the column sums reached at most 0.36 of their bound."""
import ctypes as C

import pytest
import torch

from gpu_util import (DELTA0, F8_SLOTS, F8_STRIDE, LN_BWD_CLASSES, LN_CLASSES, LN_EPS, LN_NEARCONST_SEED, LN_STAT_FLOOR, SENTINEL,
                      EXACT_LIMIT, Ln, assert_fp8_image, check_ln_elements, check_ln_partials, check_ln_stats, exact_bound,
                      exact_nt, int_operands, layernorm_bwd_fp64, layernorm_fp64, layernorm_stats_f32, ln_class_worst, ln_dy,
                      ln_fwd_cond, ln_row_bound, ln_rows, operand_values, stream)
from plbert_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT8 = 0x5A
SITE = F8_SLOTS * F8_STRIDE
PADVAL = 3e38            # input columns past H: a sum that read one would be wrecked
RESTATE_ROWS = 2304      # rows of a large case the restatement is evaluated on (256 of every class)
RSTD_ZERO = LN_EPS ** -0.5


def _affine(H, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.3 * torch.randn(H, generator=g)).to(DEV), (0.2 * torch.randn(H, generator=g)).to(DEV)


def _sentinel(t):
    return torch.tensor(SENTINEL, dtype=t.dtype, device=t.device)


def _untouched(t, what):
    assert bool((t == _sentinel(t)).all()), f"{what}: elements that must not be written were"


def _report(case, output, restated, kernel):
    for c in kernel:
        r = restated.get(c) if isinstance(restated, dict) else restated
        print(f"ln {case}: {output} class {c} restated {r:.2e} kernel {kernel[c]:.2e}")


def _two_pass_bounds(x, cls, classes):
    """(bound_mean, bound_rstd) per row and the restated per-class figures, from the two-pass restatement of (a sample of
    256 rows per class of) x."""
    n = min(x.shape[0], RESTATE_ROWS)
    st = layernorm_stats_f32(x[:n], "two_pass")
    wm, wr = ln_class_worst(st.mean_err, cls[:n], classes), ln_class_worst(st.rstd_err, cls[:n], classes)
    return ln_row_bound(wm, cls, classes, LN_STAT_FLOOR, DEV), ln_row_bound(wr, cls, classes, LN_STAT_FLOOR, DEV), wm, wr


# ------------------------------------------------------------------------------------------------ standalone forward
def _fwd_kernel_name(H, ldx, ldy):
    wide = H in (768, 1024) and ldx % 8 == 0 and ldy % 8 == 0
    return f"ln_fwd_wide_kernel<{H // 8}>" if wide else f"ln_fwd_kernel<{(H + 255) // 256}>"


def _forward(T, H, ldx=None, ldy=None, out8=False, seed=0):
    L = _lib.lib()
    ldx, ldy = ldx or H, ldy or H
    case = f"fwd {_fwd_kernel_name(H, ldx, ldy)} H {H} T {T} ld {ldx}/{ldy} out8 {int(out8)}"
    x, cls = ln_rows(T, H, 100 + seed + H + T)
    gamma, beta = _affine(H, H)
    xb = torch.full((T, ldx), PADVAL, dtype=torch.bfloat16)
    xb[:, :H] = x
    xb = xb.to(DEV)
    y = torch.full((T + 3, ldy), SENTINEL, dtype=torch.bfloat16, device=DEV)
    mean = torch.full((T + 3,), SENTINEL, device=DEV)
    rstd = torch.full((T + 3,), SENTINEL, device=DEV)
    p = _lib.PlbLayerNorm()
    p.x, p.ldx, p.gamma, p.beta, p.eps = xb.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), LN_EPS
    p.y, p.ldy, p.mean, p.rstd, p.T, p.H, p.Tzero = y.data_ptr(), ldy, mean.data_ptr(), rstd.data_ptr(), T, H, T
    if out8:
        ld8 = H + 16
        img = torch.full((T + 3, ld8), SENT8, dtype=torch.uint8, device=DEV)
        qs = torch.tensor([4.0], device=DEV)
        site = torch.zeros(SITE, device=DEV)
        p.out8, p.ld8, p.q_scale, p.q_amax = img.data_ptr(), ld8, qs.data_ptr(), site.data_ptr()
    assert L.plb_launch_ln_fwd(C.byref(p), stream()) == 0, case
    torch.cuda.synchronize()
    xd = xb[:, :H]
    rm, rr, xhat, ry = layernorm_fp64(xd, gamma, beta)
    shares = check_ln_elements(case + ": y", y[:T, :H], ry, ln_fwd_cond(xhat, gamma, beta, rm, rr), DELTA0, cls)
    bm, br, wm, wr = _two_pass_bounds(x, cls, LN_CLASSES)
    em, es = check_ln_stats(case, mean[:T], rstd[:T], xd, bm, br, cls)
    zero = (cls == LN_CLASSES.index("zero")).to(DEV)
    if bool(zero.any()):
        assert torch.equal(y[:T, :H][zero], beta.to(torch.bfloat16).expand(int(zero.sum()), H)), case + ": zero rows: y != bf16(beta)"
        assert bool(((rstd[:T][zero].double() / RSTD_ZERO - 1.0).abs() <= LN_STAT_FLOOR).all()), case + ": zero rows: rstd"
    _untouched(y[T:], case + ": y rows past T")
    _untouched(y[:T, H:], case + ": y columns past H")
    _untouched(mean[T:], case + ": mean past T")
    _untouched(rstd[T:], case + ": rstd past T")
    if out8:
        assert_fp8_image(img, y[:T], qs, 0, slice(0, T), amax_site=site, sentinel=SENT8, cols=H)
    _report(case, "y (share of delta)", DELTA0, shares)
    _report(case, "rstd", wr, ln_class_worst(es.cpu(), cls, LN_CLASSES))
    _report(case, "mean", wm, ln_class_worst(em.cpu(), cls, LN_CLASSES))


T_GRID = (1, 2, 3, 5, 9, 37)
H_GRID = (4, 64, 132, 256, 260, 512, 516, 768, 1020, 1024)


@pytest.mark.parametrize("H", H_GRID, ids=[f"H{H}-{_fwd_kernel_name(H, H, H)}" for H in H_GRID])
def test_forward_elements(H):
    """The H x T grid: every chunk count of the 8-byte kernel with full and part-empty last chunks (c < H), the 16-byte
    kernels' row groups with clamped rows (T = 1, 3, 5, 9, 37 end inside a group of 2 x 2 resp. 1 x 2 rows)."""
    for T in T_GRID:
        _forward(T, H)


@pytest.mark.parametrize("out8", [False, True], ids=["bf16", "out8"])
@pytest.mark.parametrize("H", [768, 1024], ids=["ln_fwd_wide_kernel<96>", "ln_fwd_wide_kernel<128>"])
def test_forward_wide_strides_and_image(H, out8):
    """ldx = ldy = H + 8 keeps the 16-byte kernels; with out8 the e4m3 image of y leaves too (assert_fp8_image) and y, mean,
    rstd are held to the same element contract."""
    for T in T_GRID:
        _forward(T, H, out8=out8)
        _forward(T, H, H + 8, H + 8, out8=out8)


@pytest.mark.parametrize("H", [768, 1024], ids=["ln_fwd_kernel<3>", "ln_fwd_kernel<4>"])
def test_forward_odd_stride_falls_to_the_8_byte_kernels(H):
    """ldx = H + 4: rows are no longer 16-byte aligned, the launcher must take ln_fwd_kernel<3 | 4> — same contract (the
    16-byte kernel on such rows would fault or read the neighbours' columns); out8 is refused there."""
    assert _fwd_kernel_name(H, H + 4, H) == f"ln_fwd_kernel<{H // 256}>"
    for T in (3, 37):
        _forward(T, H, H + 4, H)
        _forward(T, H, H + 4, H + 4)
    L = _lib.lib()
    p = _lib.PlbLayerNorm()
    buf = torch.zeros(8 * (H + 16), device=DEV)
    p.x, p.ldx, p.gamma, p.beta, p.eps = buf.data_ptr(), H + 4, buf.data_ptr(), buf.data_ptr(), LN_EPS
    p.y, p.ldy, p.mean, p.rstd, p.T, p.H, p.Tzero = buf.data_ptr(), H, buf.data_ptr(), buf.data_ptr(), 2, H, 2
    p.out8, p.ld8, p.q_scale = buf.data_ptr(), H, buf.data_ptr()
    assert L.plb_launch_ln_fwd(C.byref(p), stream()) != 0


@pytest.mark.parametrize("out8", [False, True], ids=["bf16", "out8"])
@pytest.mark.parametrize("H,T", [(768, 32768 + 5), (1024, 16384 + 3)], ids=["ln_fwd_wide_kernel<96>", "ln_fwd_wide_kernel<128>"])
def test_forward_second_grid_stride_iteration(H, T, out8):
    """2048 workgroups x 4 waves x (2 x 2 | 1 x 2) rows = 32768 | 16384 rows per grid-stride iteration: the rows past that
    are the second iteration, and its last group is clamped."""
    _forward(T, H, out8=out8)


# ------------------------------------------------------------------------------------------------ standalone backward
def _bwd_kernel_name(H, ldx, lddy, lddx, out8):
    wide_ok = H in (768, 1024) and ldx % 8 == 0 and lddy % 8 == 0 and lddx % 8 == 0
    return f"ln_bwd_wide_kernel<{H // 8}>" if wide_ok and (out8 or H == 1024) else f"ln_bwd_kernel<{(H + 255) // 256}>"


def _backward(T, H, nblocks, ldx=None, lddy=None, lddx=None, out8=False, accumulate=False):
    L = _lib.lib()
    ldx, lddy, lddx = ldx or H, lddy or H, lddx or H
    kname = _bwd_kernel_name(H, ldx, lddy, lddx, out8)
    case = f"bwd {kname} H {H} T {T} nblocks {nblocks} ld {ldx}/{lddy}/{lddx} out8 {int(out8)}"
    Tzero = T + 3
    x, cls = ln_rows(T, H, 200 + H + T, LN_BWD_CLASSES)
    dy, kind = ln_dy(T, H, 300 + H + T)
    gamma, _ = _affine(H, H + 1)
    xb = torch.full((T, ldx), PADVAL, dtype=torch.bfloat16)
    xb[:, :H] = x
    dyb = torch.full((T, lddy), PADVAL, dtype=torch.bfloat16)
    dyb[:, :H] = dy
    xb, dyb = xb.to(DEV), dyb.to(DEV)
    m64, r64, _, _ = layernorm_fp64(xb[:, :H], gamma, torch.zeros_like(gamma))
    mean, rstd = m64.float(), r64.float()                        # the statistics a forward stores: fp32
    dx = torch.full((Tzero + 3, lddx), SENTINEL, dtype=torch.bfloat16, device=DEV)
    part = torch.full((nblocks, 3 * H), 9.0, device=DEV)          # accumulate = 0 must overwrite
    p = _lib.PlbLayerNorm()
    p.x, p.ldx, p.gamma, p.eps = xb.data_ptr(), ldx, gamma.data_ptr(), LN_EPS
    p.mean, p.rstd, p.T, p.H, p.Tzero = mean.data_ptr(), rstd.data_ptr(), T, H, Tzero
    p.dy, p.lddy, p.dx, p.lddx, p.partials, p.nblocks = dyb.data_ptr(), lddy, dx.data_ptr(), lddx, part.data_ptr(), nblocks
    if out8:
        ld8 = H + 16
        img = torch.full((Tzero + 3, ld8), SENT8, dtype=torch.uint8, device=DEV)
        qs = torch.tensor([64.0], device=DEV)
        site = torch.zeros(SITE, device=DEV)
        p.out8, p.ld8, p.q_scale, p.q_amax = img.data_ptr(), ld8, qs.data_ptr(), site.data_ptr()
    assert L.plb_launch_ln_bwd(C.byref(p), stream()) == 0, case
    torch.cuda.synchronize()
    first = (dx.clone(), part.clone(), img.clone() if out8 else None)
    ref = layernorm_bwd_fp64(xb[:, :H], mean, rstd, gamma, dyb[:, :H])
    shares = check_ln_elements(case + ": dx", dx[:T, :H], ref.dx, ref.cond, DELTA0, cls, LN_BWD_CLASSES)
    assert bool((dx[:T, :H][(kind == 3).to(DEV)] == 0).all()), case + ": an all-zero dy row must leave an exactly zero dx row"
    assert bool((dx[T:Tzero, :H] == 0).all()), case + ": rows T..Tzero of dx are zero"
    _untouched(dx[Tzero:], case + ": dx rows past Tzero")
    _untouched(dx[:, H:], case + ": dx columns past H")
    # the partial rows: a workgroup without rows leaves exact zeros (not the 9.0 it found); summed in float64 they are the
    # column sums. rows per lane: wave w of workgroup b takes rows (4 b + w) x RW + 4 RW nblocks k
    rw = 2 if kname == "ln_bwd_wide_kernel<96>" else 1
    fed = min(nblocks, -(-T // (4 * rw)))
    empty = int((part == 0).all(1).sum())
    assert empty >= nblocks - fed, f"{case}: {nblocks - fed} workgroups have no rows, {empty} partial rows are zero"
    sums = part.double().sum(0)
    stored = dx[:T, :H].double()
    rpl = -(-T // (4 * nblocks))
    ratios = {}
    for k, (what, want, mag) in enumerate((("dgamma", ref.dgamma, ref.mag_gamma), ("dbeta", ref.dbeta, ref.mag_beta),
                                           ("colsum(dx)", stored.sum(0), stored.abs().sum(0)))):
        ratios[what] = check_ln_partials(f"{case}: {what}", sums[k * H:(k + 1) * H], want, mag, rpl)
    if out8:
        im = img.cpu()
        assert bool((im[T:Tzero, :H] == 0).all()), case + ": image rows T..Tzero are zero bytes"
        im[T:Tzero, :H] = SENT8
        assert_fp8_image(im, dx[:T], qs, 1, slice(0, T), amax_site=site, sentinel=SENT8, cols=H)
    # a second launch: bitwise the same; with accumulate = 1: partials == first + first (one fp32 add per word)
    p.accumulate = int(accumulate)
    assert L.plb_launch_ln_bwd(C.byref(p), stream()) == 0, case
    torch.cuda.synchronize()
    assert torch.equal(dx, first[0]), case + ": dx of a second launch differs"
    assert torch.equal(part, first[1] + first[1] if accumulate else first[1]), case + f": partials, accumulate {int(accumulate)}"
    if out8:
        assert torch.equal(img, first[2]), case + ": image of a second launch differs"
    _report(case, "dx (share of delta)", DELTA0, shares)
    print(f"ln {case}: column sums err / bound " + " ".join(f"{k} {v:.2f}" for k, v in ratios.items()))


BWD_IDS = [f"H{H}-{_bwd_kernel_name(H, H, H, H, False)}" for H in H_GRID]


@pytest.mark.parametrize("H", H_GRID, ids=BWD_IDS)
def test_backward_elements(H):
    """The H x T grid with nblocks 1 (every row behind one lane set), 3, and 64 (workgroups without rows at T <= 37)."""
    for T in T_GRID:
        for nblocks in (1, 3, 64):
            _backward(T, H, nblocks, accumulate=(nblocks == 3))


@pytest.mark.parametrize("H", [768, 1024], ids=["ln_bwd_kernel<3>", "ln_bwd_wide_kernel<128>"])
def test_backward_strides(H):
    """lddy != lddx != ldx, all multiples of 8 (H = 1024 stays in the 16-byte kernel), then ldx = H + 4, which must fall
    to ln_bwd_kernel<3 | 4>."""
    for T in (5, 37):
        _backward(T, H, 3, H + 8, H + 16, H + 24)
        assert _bwd_kernel_name(H, H + 4, H + 16, H + 24, False) == f"ln_bwd_kernel<{H // 256}>"
        _backward(T, H, 3, H + 4, H + 16, H + 24)


@pytest.mark.parametrize("T", [1, 5, 333])
@pytest.mark.parametrize("H", [768, 1024], ids=["ln_bwd_wide_kernel<96>", "ln_bwd_wide_kernel<128>"])
def test_backward_wide_with_image(H, T):
    """out8: the only way into ln_bwd_wide_kernel<96> (H = 768: load 1 of a lane straddles two rows, the column sums leave
    through a three-stage LDS fold). dx, dgamma, dbeta and the column sums against float64, the e5m2 image against dx."""
    for nblocks in (1, 3, 64):
        _backward(T, H, nblocks, out8=True, accumulate=(nblocks == 64))
    _backward(T, H, 3, H + 8, H + 16, H + 24, out8=True)


# ------------------------------------------------------------------------------------------------------- fused forms
FUSED_N = (256, 384, 512, 768, 1024, 1152, 1536)          # 1, 1, 2, 2, 4, 3, 4 column tiles
FUSED_M = 1024
NO_GEMM = ("small", "eps", "zero", "nearconst")           # rows whose A row is zero: the GEMM term would swamp the class
FP8_LN_DEQ = (2.0 ** -3, 2.0 ** -4)


def _tile(N):
    return 384 if N % 384 == 0 else 256


def _fused_inputs(N, fp8, seed, a_bf8, zero_rows):
    """Integer operands (exact in any order): A in [-4, 4] with the rows in zero_rows zeroed, B in [-4, 4] x 2^-6 (bf16) or
    in [-4, 4] with dequantisation factors 2^-3 x 2^-4 (fp8): A.B^T has a standard deviation of 0.8 / 0.6 and is a multiple
    of 2^-6 / 2^-7. Returns device operands, their values and the exact product in float64."""
    M, K = FUSED_M, (128 if fp8 else 64)
    ka = ("e5m2" if a_bf8 else "e4m3") if fp8 else "bf16"
    kb = "e4m3" if fp8 else "bf16"
    A = int_operands((M, K), -4, 4, seed, ka)
    A[zero_rows] = 0
    B = int_operands((N, K), -4, 4, seed + 1, kb, 1.0 if fp8 else 2.0 ** -6)
    Av, Bv = operand_values(A, ka), operand_values(B, kb)
    scale = FP8_LN_DEQ[0] * FP8_LN_DEQ[1] if fp8 else 1.0
    unit = scale if fp8 else 2.0 ** -6
    assert exact_bound(Av, Bv, unit=1.0 if fp8 else unit) < EXACT_LIMIT
    return A.to(DEV), B.to(DEV), exact_nt(Av, Bv, scale=scale).to(DEV), K


def _ln_launch(t, p, mode, fp8, a_bf8):
    L = _lib.lib()
    if fp8:
        deq = torch.tensor(FP8_LN_DEQ, dtype=torch.float32, device=DEV)
        p.deq_a, p.deq_b = deq.data_ptr(), deq.data_ptr() + 4
        rc = L.plb_launch_gemm_nt_fp8_ln(C.byref(p), mode, int(a_bf8), stream())
    else:
        rc = L.plb_launch_gemm_nt_ln(C.byref(p), mode, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(t.err.item()) == 0, "a hand-off timed out"
    assert int(t.xchg.abs().sum().item()) == 0, "hand-off words left set"


def _fused_forward(N, fp8, bias_const, Mstore, res_cls=None, case_tag=""):
    M, TN = FUSED_M, _tile(N)
    case = f"fused form 5 {'fp8' if fp8 else 'bf16'} tile {TN} N {N} bias {bias_const:g} Mstore {Mstore}{case_tag}"
    res, cls = res_cls if res_cls is not None else ln_rows(M, N, 400 + N)
    classes = LN_CLASSES if res_cls is None else ("nearconst",)
    no_gemm = torch.tensor([classes[int(c)] in NO_GEMM for c in cls])
    A, B, acc, K = _fused_inputs(N, fp8, 500 + N, 0, no_gemm)
    t = Ln(M, N, K, seed=N)
    t.A, t.B = A, B
    t.bias = torch.full((N,), float(bias_const), device=DEV)
    t.res = res.to(DEV)
    # known without the kernel: the integer product is exact in fp32, then the epilogue's two fp32 additions in its order
    # (+ bias, + residual), then one round-to-nearest-even to bf16
    want_pre = ((acc.float() + t.bias) + t.res.float()).to(torch.bfloat16)
    pre = torch.full((M, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    y = torch.full((M, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    t.mean.fill_(SENTINEL)
    t.rstd.fill_(SENTINEL)
    p = t.params()
    p.A, p.B, p.Mstore = A.data_ptr(), B.data_ptr(), Mstore
    p.bias, p.res, p.ldr = t.bias.data_ptr(), t.res.data_ptr(), N
    p.C, p.ldc, p.C2, p.ldc2 = pre.data_ptr(), N, y.data_ptr(), N
    if fp8:
        img = torch.full((M, N), SENT8, dtype=torch.uint8, device=DEV)
        qs = torch.tensor([4.0], device=DEV)
        site = torch.zeros(SITE, device=DEV)
        p.C8, p.ldc8, p.q_scale, p.q_amax = img.data_ptr(), N, qs.data_ptr(), site.data_ptr()
    _ln_launch(t, p, 5, fp8, 0)
    ms = Mstore
    assert torch.equal(pre[:ms], want_pre[:ms]), case + ": the premise: pre is the exact sum, rounded once"
    for o, what in ((pre, "pre"), (y, "y"), (t.mean, "mean"), (t.rstd, "rstd")):
        _untouched(o[ms:], f"{case}: {what} rows past Mstore")
    if fp8:
        assert_fp8_image(img, y[:ms], qs, 0, slice(0, ms), amax_site=site, sentinel=SENT8)
    x = want_pre[:ms]
    cl = cls[:ms]
    mean, rstd = t.mean[:ms], t.rstd[:ms]
    assert bool(torch.isfinite(mean).all() and torch.isfinite(rstd).all() and torch.isfinite(y[:ms].float()).all()), case + ": not finite"
    assert bool(((rstd > 0) & (rstd.double() <= RSTD_ZERO * (1 + LN_STAT_FLOOR))).all()), case + ": rstd outside (0, eps^-1/2]"
    if "nearconst" in classes:
        keep = cl != classes.index("nearconst")                   # no relative bound there (finite, rstd in range: above)
        if not bool(keep.any()):
            n_bad = int((layernorm_stats_f32(x.cpu(), ("tile", TN)).m2 <= 0).sum())
            print(f"ln {case}: y class nearconst restated {n_bad} rows with m2 <= 0 kernel all finite, rstd max {float(rstd.max()):.4e}")
            return
    else:
        keep = torch.ones(ms, dtype=torch.bool)
    idx = keep.nonzero().flatten()
    xk, ck = x[idx.to(DEV)], cl[idx]
    st = layernorm_stats_f32(xk.cpu(), ("tile", TN))
    wm, wr = ln_class_worst(st.mean_err, ck, classes), ln_class_worst(st.rstd_err, ck, classes)
    rm, rr, xhat, ry = layernorm_fp64(xk, t.gamma, t.beta)
    delta = ln_row_bound(wr, ck, classes, DELTA0, DEV)            # per class: max(DELTA0, 4 x restated)
    shares = check_ln_elements(case + ": y", y[:ms][idx.to(DEV)], ry, ln_fwd_cond(xhat, t.gamma, t.beta, rm, rr), delta, ck, classes)
    em, es = check_ln_stats(case, mean[idx.to(DEV)], rstd[idx.to(DEV)], xk, ln_row_bound(wm, ck, classes, LN_STAT_FLOOR, DEV),
                            ln_row_bound(wr, ck, classes, LN_STAT_FLOOR, DEV), ck, classes)
    const = (xk == xk[:, :1]).all(1) & (xk[:, 0] == 0)
    if bool(const.any()):                                          # all-zero rows (bias 0): y == bf16(beta), rstd = eps^-1/2
        yk = y[:ms][idx.to(DEV)]
        assert torch.equal(yk[const], t.beta.to(torch.bfloat16).expand(int(const.sum()), N)), case + ": zero rows: y != bf16(beta)"
        assert bool(((rstd[idx.to(DEV)][const].double() / RSTD_ZERO - 1.0).abs() <= LN_STAT_FLOOR).all()), case + ": zero rows: rstd"
    _report(case, "y (share of delta)", {c: max(DELTA0, 4 * wr[c]) for c in wr}, shares)
    _report(case, "rstd", wr, ln_class_worst(es.cpu(), ck, classes))
    _report(case, "mean", wm, ln_class_worst(em.cpu(), ck, classes))


def _fused_backward(N, fp8, Mstore):
    M, TN = FUSED_M, _tile(N)
    case = f"fused form 6 {'fp8 LEAN' if fp8 else 'bf16'} tile {TN} N {N} Mstore {Mstore}"
    aux, cls = ln_rows(M, N, 600 + N, LN_BWD_CLASSES)
    res, kind = ln_dy(M, N, 700 + N)
    A, B, acc, K = _fused_inputs(N, fp8, 800 + N, 1, (kind == 1) | (kind == 3))   # tiny and zero dy rows: no GEMM term
    t = Ln(M, N, K, seed=N + 1)
    t.A, t.B, t.res = A, B, res.to(DEV)
    aux = aux.to(DEV)
    dy = (acc.float() + t.res.float()).to(torch.bfloat16)         # known without the kernel (the epilogue's one fp32 addition)
    m64, r64, _, _ = layernorm_fp64(aux, t.gamma, t.beta)
    t.mean.copy_(m64.float())
    t.rstd.copy_(r64.float())
    dx = torch.full((M, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    colp = torch.full((2 * M // 128, 3, N), 9.0, dtype=torch.float32, device=DEV)
    p = t.params()
    p.A, p.B, p.Mstore = A.data_ptr(), B.data_ptr(), Mstore
    p.res, p.ldr, p.aux, p.ldaux = t.res.data_ptr(), N, aux.data_ptr(), N
    p.C, p.ldc, p.colpart = dx.data_ptr(), N, colp.data_ptr()
    if fp8:
        img = torch.full((M, N), SENT8, dtype=torch.uint8, device=DEV)
        qs = torch.tensor([64.0], device=DEV)
        site = torch.zeros(SITE, device=DEV)
        p.C8, p.ldc8, p.q_scale, p.q_amax = img.data_ptr(), N, qs.data_ptr(), site.data_ptr()
    _ln_launch(t, p, 6, fp8, 1)
    ms = Mstore
    ref = layernorm_bwd_fp64(aux, t.mean, t.rstd, t.gamma, dy)   # over ALL M rows
    shares = check_ln_elements(case + ": dx", dx[:ms], ref.dx[:ms], ref.cond[:ms], DELTA0, cls[:ms], LN_BWD_CLASSES)
    assert bool((dx[:ms][(kind[:ms] == 3).to(DEV)] == 0).all()), case + ": an all-zero dy row must leave an exactly zero dx row"
    _untouched(dx[ms:], case + ": dx rows past Mstore")
    if fp8:
        assert_fp8_image(img, dx[:ms], qs, 1, slice(0, ms), amax_site=site, sentinel=SENT8)
    # [2 M / 128][3][N]: one partial row per 64 rows, 4 rows per lane, the rest a tree; summed here in float64.
    # dgamma / dbeta run over ALL M rows — the kernel does not mask dg / db by Mstore (rows past it are computed, only never
    # stored: the engine's padded rows carry dy = 0) — the column sums of dx over the stored rows only.
    sums = colp.double().sum(0)
    stored = dx[:ms].double()
    ratios = {}
    for k, (what, want, mag) in enumerate((("dgamma", ref.dgamma, ref.mag_gamma), ("dbeta", ref.dbeta, ref.mag_beta),
                                           ("colsum(dx)", stored.sum(0), stored.abs().sum(0)))):
        ratios[what] = check_ln_partials(f"{case}: {what}", sums[k], want, mag, 4)
    _report(case, "dx (share of delta)", DELTA0, shares)
    print(f"ln {case}: column sums err / bound " + " ".join(f"{k} {v:.2f}" for k, v in ratios.items()))


def _fused_id(N):
    return f"N{N}-tile{_tile(N)}x{N // _tile(N)}"


@pytest.mark.parametrize("fp8", [False, True], ids=["gemm_ln-bf16-form5", "gemm_fp8_ln-fp8-form5"])
@pytest.mark.parametrize("N", FUSED_N, ids=[_fused_id(N) for N in FUSED_N])
def test_fused_forward_elements(N, fp8):
    """Form 5. The residual carries the classes; the bias is a constant (0: the classes as they are; 2: offsets from bias
    AND residual — the small / eps / zero rows then round to exactly constant rows, variance 0); then Mstore = M - 300."""
    for bias_const, Mstore in ((0.0, FUSED_M), (2.0, FUSED_M), (2.0, FUSED_M - 300)):
        _fused_forward(N, fp8, bias_const, Mstore)


@pytest.mark.parametrize("fp8", [False, True], ids=["gemm_ln-bf16-form5", "gemm_fp8_ln-fp8-form5"])
@pytest.mark.parametrize("N", [768, 1024, 1152], ids=[_fused_id(N) for N in (768, 1024, 1152)])
def test_fused_forward_near_constant_rows(N, fp8):
    """1024 near-constant rows from the committed seed (at N = 768 the restatement's merged M2 is <= 0 on some of them):
    mean, rstd and every y finite and 0 < rstd <= eps^-1/2 (1 + 2^-20). One-pass arithmetic cannot resolve such a row, so
    no relative bound is asked. Without the clamp of m2 in csrc/gemm_nt_pipeline.h a negative M2 is a NaN row."""
    rows = ln_rows(FUSED_M, N, LN_NEARCONST_SEED, ("nearconst",))
    _fused_forward(N, fp8, 0.0, FUSED_M, res_cls=rows, case_tag=" nearconst")


@pytest.mark.parametrize("fp8", [False, True], ids=["gemm_ln-bf16-form6", "gemm_fp8_ln-fp8-form6-LEAN"])
@pytest.mark.parametrize("N", FUSED_N, ids=[_fused_id(N) for N in FUSED_N])
def test_fused_backward_elements(N, fp8):
    """Form 6: dy = bf16(A.B^T + res) (fp8: A in e5m2, the LEAN epilogue), aux the pre-LayerNorm rows of six classes, their
    fp32 statistics from float64; then Mstore = M - 300."""
    for Mstore in (FUSED_M, FUSED_M - 300):
        _fused_backward(N, fp8, Mstore)
