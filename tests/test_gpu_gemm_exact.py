"""-m gpu: the GEMM family held BIT FOR BIT with small-integer operands.

The aggregate tests (test_gpu_kernels.py, test_gpu_gemm_ln.py, test_gpu_fp8.py: rel_l2 < 4e-3 in bf16, < 1e-5 in fp32) cannot
see a K-tile dropped in one 16x16 MFMA patch, a fragment read from the wrong ring slot once per launch or a residual read
at the wrong row stride: at the engine's shapes such a defect is diluted far under the line. With operands that are
integers in [-4, 4] (exact in bf16, e4m3 and e5m2), an integer bias in [-64, 64] and an integer bf16 residual in
[-128, 128], every product and every partial sum is an exact fp32 number as long as gpu_util.exact_bound — the largest sum
of the terms' magnitudes — stays below 2^24; every case asserts that before it launches (a condition, not a tolerance). The
result then does not depend on summation order, tile form, K-loop form or split count: fp32 outputs must EQUAL the float64
reference and bf16 outputs its round-to-nearest-even (torch.equal semantics: the sign of zero is not part of the
contract). The assertion message is gpu_util.first_mismatch's: how many elements differ, the first one, its row tile,
column tile and 64x32 wave patch. tests/test_gemm_exact_host.py proves the method and the checker on the CPU; the case
tables live in gpu_util (NT_FORMS, NT_TAILS, FP8_NT_FORMS, LN_CASES, CE_*, TN_*).

What is NOT bitwise: the gelu epilogues evaluate gelu_new / gelu_new' in fp32 with v_exp_f32 / v_rcp_f32. On exact
pre-activations (B x 2^-4, so that u lands in gelu's active range) they are held to two derived allowances:
    act 1   C = RNE(u) bit for bit; |C2 - gelu64(C)| <= one bf16 spacing of the reference (floor 2^-64)
    act 2   |C - v gelu'64(aux)| <= one bf16 spacing of the reference + |v| 2^-16   (v the exact accumulator)
At aux = +16 / -16 the fp32 evaluation saturates and gelu' is exactly 1 / 0: the act 2 launches of the bitwise tests use
only those two values, which keeps their outputs and column sums exact.

THE KERNELS' FIGURES ARE STILL MISSING: no MI355X could be had while this module was written, so it has not run on one yet
(its logic ran on the CPU against an exact emulation of the launchers). The first -s run prints, per form, `gelu form <f>:
act 1 <fraction of the allowance> at <element>: u .., C2 .. | act 2 <fraction> at <element>: v .., aux .., C .., reference ..`;
those fractions belong here, next to the host restatement's (tests/test_gemm_exact_host.py: gelu 0.4998 of a bf16 spacing,
gelu' 1.9e-6 absolute; an emulation that rounds the restatement to bf16 gives 0.4974 for act 1 and 0.4991 for act 2).
The same holds for the premise test's outcome (test_premise_...: whether gfx950's MFMAs accumulate exact small-integer
products exactly). If it fails with the same few units in the last place in every form of one operand type, that type is
to be held to |got - ref| <= (K + 3) 2^-23 (sum |a||b| + |bias| + |res|) for fp32 outputs (+ 2^-8 |ref| for bf16 outputs)
in this whole module, and nothing wider.
"""
import contextlib
import ctypes as C

import pytest
import torch

from plbert_amd import _lib
from gpu_util import (CE_COLS, CE_SHAPE, CE_TILES, EXACT_LIMIT, FP8_DEQ, FP8_KTILES, FP8_NT_FORMS, GELU_KTILES, GELU_UNIT,
                      LN_CASES, NT_FORM_PARAMS, NT_FORMS, NT_STRIDE_KTILES, NT_TAILS, SENTINEL, TN_BIG, TN_FP8, TN_PLANNED,
                      TN_PLANNED_SPLITS, TN_SMALL, Ln,
                      assert_exact, assert_untouched, exact_bound, exact_nt, exact_tn, first_mismatch, gelu64, gelu_grad64,
                      gemm_nt, gemm_nt_fp8, gemm_tn_slabs, int_operands, nt_operands, operand_values, reduce_slabs, rne_bf16,
                      spacing_bf16, stream, tn_operands)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(*ts):
    return [t.to(DEV) if t is not None else None for t in ts]


@contextlib.contextmanager
def forced(tile, prefetch=-1):
    """The launches inside run on this tile form (and K-loop form); afterwards the per-shape policy is back."""
    L = _lib.lib()
    try:
        L.plb_set_gemm_nt_tile(tile)
        L.plb_set_gemm_nt_prefetch(prefetch)
        yield L
    finally:
        L.plb_set_gemm_nt_tile(0)
        L.plb_set_gemm_nt_prefetch(-1)


def premise(A, B, bias=None, res=None, unit=1.0):
    bound = exact_bound(A, B, bias, res, unit)
    assert bound < EXACT_LIMIT, f"the case is not exact in fp32: sum of magnitudes {bound} units"


def strided(t, ld, junk):
    """t's values in a [rows, ld] buffer whose gap columns hold junk; returns (the view of t's columns, the buffer)."""
    buf = torch.full((t.shape[0], ld), junk, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]], buf


# ---- 3.0 the premise on the hardware ----------------------------------------------------------------------------------------
def test_premise_mfma_accumulates_small_integer_products_exactly():
    """One workgroup, one K-tile, inputs in [-4, 4], per operand type: the 128 kernel and every big bf16 form in fp32 out
    (v_mfma_f32_16x16x32_bf16), the fp8 NT forms in bf16 out (they have no fp32 output) and the fp8 TN kernel in fp32 out
    (v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales). A failure HERE — the same few units in the last place in every
    form — would be the hardware's accumulation, not a kernel's K loop; everything below builds on this passing."""
    found = []

    def note(what, got, want, TM, TN):
        msg = first_mismatch(got, want, TM, TN)
        if msg:
            found.append(f"{what}: {msg}")

    for form, pf in NT_FORM_PARAMS:
        TM, TN = NT_FORMS[form][:2]
        A, B = dev(*nt_operands(TM, TN, 64, 11)[:2])
        premise(A, B)
        with forced(form, pf):
            out, _ = gemm_nt(A, B, TN, out_f32=True, fill=SENTINEL)
        note(f"bf16 operands, form {form} K-loop form {pf}, fp32 out", out, exact_nt(A, B), TM, TN)
    for form, (TM, TN, _) in FP8_NT_FORMS.items():
        for bf8, ka in ((0, "e4m3"), (1, "e5m2")):
            A8, B8 = dev(*nt_operands(TM, TN, 128, 12 + bf8, kinds=(ka, "e4m3"))[:2])
            Av, Bv = operand_values(A8, ka), operand_values(B8, "e4m3")
            premise(Av, Bv)
            out = gemm_nt_fp8(A8, B8, TN, (1.0, 1.0), a_bf8=bf8, fill=SENTINEL)
            note(f"{ka} x e4m3 operands, NT form {form}, bf16 out", out, rne_bf16(exact_nt(Av, Bv)), TM, TN)
    A8, B8 = dev(*tn_operands(128, 256, 256, 14, kinds=("e5m2", "e4m3")))
    Av, Bv = operand_values(A8, "e5m2"), operand_values(B8, "e4m3")
    premise(Av.T, Bv.T)
    slab = gemm_tn_slabs(A8, B8, 256, 1, 128, "fp8", deq=(1.0, 1.0))
    note("e5m2 x e4m3 operands, TN kernel, fp32 out", slab.reshape(256, 256), Av.T @ Bv, 256, 256)
    assert not found, "; ".join(found)


# ---- 3a NT, bitwise ---------------------------------------------------------------------------------------------------------
def saturated_aux(M, N, seed):
    """aux in {-16, +16}: gelu_new' evaluates to exactly 0 / 1 there (the exponential over- / underflows). -> (aux, 0/1)."""
    keep = int_operands((M, N), 0, 1, seed, "f32").to(DEV)
    return (keep * 32.0 - 16.0).to(torch.bfloat16), keep.double()


def check_colpart(L, A, B, N, TM, TN, act, ms, want, what, **kw):
    """The launch with column-sum partials against the one without (bit for bit, sentinel rows included), both against
    `want` on the stored rows; colpart[2t] + colpart[2t+1] == the column sums of the stored bf16 rows of row tile t."""
    M = A.shape[0]
    nrt = M // TM
    assert L.plb_gemm_nt_colpart_rows(M, N, A.shape[1]) == 2 * nrt
    plain, _ = gemm_nt(A, B, N, act=act, Mstore=ms, fill=SENTINEL, **kw)
    cp = torch.full((2 * nrt, N), SENTINEL, dtype=torch.float32, device=DEV)
    withcp, _ = gemm_nt(A, B, N, act=act, Mstore=ms, fill=SENTINEL, colpart=cp, **kw)
    assert_exact(plain[:ms], want[:ms], TM, TN, f"{what}, no colpart")
    assert_untouched(plain[ms:], f"{what}, no colpart, rows >= Mstore")
    assert_exact(withcp, plain, TM, TN, f"{what}: the colpart launch's output against the plain launch's")
    stored = withcp.double()
    stored[ms:] = 0.0
    tiles = stored.reshape(nrt, TM, N)
    assert float(tiles.abs().sum(1).max()) < EXACT_LIMIT
    assert_exact(cp.double().reshape(nrt, 2, N).sum(1), tiles.sum(1), 1, TN, f"{what}: colpart pair sums (row = row tile)")


def check_strided(form, TM, TN, A, B, bias, res, what):
    """lda = K + 8, ldb = K + 16, ldr = N + 8, ldaux = N + 12, ldc = ldc2 = ldcf = N + 4: gap elements of the inputs hold
    non-zero junk, gap elements of the outputs keep their sentinel, stored values are bit-equal."""
    M, K = A.shape
    N = B.shape[0]
    As, _ = strided(A, K + 8, 2.5)
    Bs, _ = strided(B, K + 16, -1.5)
    Rs, _ = strided(res, N + 8, 3.5)
    ld = dict(ldc=N + 4, ldc2=N + 4, ldcf=N + 4, fill=SENTINEL)
    out, _ = gemm_nt(As, Bs, N, bias=bias, res=Rs, **ld)
    assert_exact(out[:, :N], rne_bf16(exact_nt(A, B, bias, res)), TM, TN, f"{what} act 0")
    assert_untouched(out[:, N:], f"{what} act 0, gap of C")
    outf, _ = gemm_nt(As, Bs, N, bias=bias, out_f32=True, **ld)
    assert_exact(outf[:, :N], exact_nt(A, B, bias), TM, TN, f"{what} fp32 out")
    assert_untouched(outf[:, N:], f"{what} gap of Cf")
    u, g = gemm_nt(As, Bs, N, bias=bias, act=1, **ld)
    assert_exact(u[:, :N], rne_bf16(exact_nt(A, B, bias)), TM, TN, f"{what} act 1, C")
    over = gelu_excess(g[:, :N], u[:, :N])
    assert float(over.max()) <= 1.0, f"{what} act 1, C2: {float(over.max())} of the allowance"
    assert_untouched(u[:, N:], f"{what} act 1, gap of C")
    assert_untouched(g[:, N:], f"{what} act 1, gap of C2")
    aux, keep = saturated_aux(M, N, 31)
    Xs, _ = strided(aux, N + 12, 0.75)
    du, _ = gemm_nt(As, Bs, N, aux=Xs, act=2, **ld)
    assert_exact(du[:, :N], rne_bf16(exact_nt(A, B) * keep), TM, TN, f"{what} act 2")
    assert_untouched(du[:, N:], f"{what} act 2, gap of C")


@pytest.mark.parametrize("form,pf", NT_FORM_PARAMS)
def test_nt_bitwise(form, pf):
    TM, TN, (M, N), ktiles = NT_FORMS[form]
    for kt in ktiles:
        A, B, bias, res = dev(*nt_operands(M, N, 64 * kt, 1000 * form + kt))
        premise(A, B, bias, res)
        want, wantf = rne_bf16(exact_nt(A, B, bias, res)), exact_nt(A, B, bias)
        what = f"form {form} K-loop form {pf}, {kt} K-tiles"
        with forced(form, pf) as L:
            out, _ = gemm_nt(A, B, N, bias=bias, res=res, fill=SENTINEL)
            assert_exact(out, want, TM, TN, f"{what}, act 0 + bias + res")
            buf = res.clone()
            out, _ = gemm_nt(A, B, N, bias=bias, res=buf, C=buf)
            assert_exact(out, want, TM, TN, f"{what}, act 0 + bias + res IN PLACE")
            for ms in (M - 5, TM + 3, 1):
                outf, _ = gemm_nt(A, B, N, bias=bias, out_f32=True, Mstore=ms, fill=SENTINEL)
                assert_exact(outf[:ms], wantf[:ms], TM, TN, f"{what}, fp32 out, Mstore {ms}")
                assert_untouched(outf[ms:], f"{what}, fp32 out, rows >= Mstore {ms}")
            if form != 128:   # column-sum partials exist in the big-tile kernels only
                aux, keep = saturated_aux(M, N, 30 + kt)
                want2 = rne_bf16(exact_nt(A, B) * keep)
                for ms in (M, TM + 3):
                    check_colpart(L, A, B, N, TM, TN, 0, ms, want, f"{what}, act 0, Mstore {ms}", bias=bias, res=res)
                    check_colpart(L, A, B, N, TM, TN, 2, ms, want2, f"{what}, act 2, Mstore {ms}", aux=aux)
            if kt == NT_STRIDE_KTILES:
                check_strided(form, TM, TN, A, B, bias, res, f"{what}, strided")


@pytest.mark.parametrize("M,N", NT_TAILS)
def test_nt_128_column_tails(M, N):
    """N off the 128-column tile: B has ceil128(N) rows and the rows past N hold 3, not zero; C has ldc = N + 4 and a
    sentinel. Nothing of the pad rows may appear and nothing past column N may be written."""
    for kt in NT_FORMS[128][3]:
        A, B, bias, res = dev(*nt_operands(M, N, 64 * kt, 2000 + N + kt, brows=(N + 127) // 128 * 128))
        B[N:] = 3.0
        premise(A, B[:N], bias, res)
        what = f"128 kernel {M} x {N}, {kt} K-tiles"
        with forced(128):
            out, _ = gemm_nt(A, B, N, bias=bias, res=res, ldc=N + 4, fill=SENTINEL)
            outf, _ = gemm_nt(A, B, N, bias=bias, out_f32=True, ldcf=N + 4, Mstore=M - 5, fill=SENTINEL)
        assert_exact(out[:, :N], rne_bf16(exact_nt(A, B[:N], bias, res)), 128, 128, what)
        assert_untouched(out[:, N:], f"{what}, past column N")
        assert_exact(outf[:M - 5, :N], exact_nt(A, B[:N], bias)[:M - 5], 128, 128, f"{what}, fp32 out")
        assert_untouched(outf[:, N:], f"{what}, fp32 out, past column N")
        assert_untouched(outf[M - 5:], f"{what}, fp32 out, rows >= Mstore")


@pytest.mark.parametrize("bf8", [0, 1])
@pytest.mark.parametrize("form", list(FP8_NT_FORMS))
def test_nt_fp8_bitwise(form, bf8):
    """1-byte operands, deq_a = 2^-3, deq_b = 2^-2: C = RNE((A.B^T) 2^-5 + bias + res), in place too."""
    TM, TN, (M, N) = FP8_NT_FORMS[form]
    ka = "e5m2" if bf8 else "e4m3"
    for kt in FP8_KTILES:
        A8, B8, bias, res = dev(*nt_operands(M, N, 128 * kt, 3000 + form + 10 * kt + bf8, kinds=(ka, "e4m3")))
        Av, Bv = operand_values(A8, ka) * FP8_DEQ[0], operand_values(B8, "e4m3") * FP8_DEQ[1]
        premise(Av, Bv, bias, res, unit=FP8_DEQ[0] * FP8_DEQ[1])
        want = rne_bf16(exact_nt(Av, Bv, bias, res))
        what = f"fp8 form {form}, A {ka}, {kt} K-tiles of 128"
        out = gemm_nt_fp8(A8, B8, N, FP8_DEQ, bias, res, bf8, fill=SENTINEL)
        assert_exact(out, want, TM, TN, what)
        buf = res.clone()
        assert_exact(gemm_nt_fp8(A8, B8, N, FP8_DEQ, bias, buf, bf8, C=buf), want, TM, TN, f"{what} IN PLACE")


@pytest.mark.parametrize("M,N,K", LN_CASES)
def test_layernorm_form_stores_the_exact_sum(M, N, K):
    """Form 5 (GEMM + LayerNorm forward): the stored pre-LayerNorm sum is the integer reference's RNE, no hand-off timed
    out and the hand-off words are back at zero; with fp8 operands too where K % 128 allows."""
    L = _lib.lib()
    TN = 384 if N % 384 == 0 else 256
    for fp8 in ((False, True) if K % 128 == 0 else (False,)):
        t = Ln(M, N, K)
        A, B, t.bias, t.res = dev(*nt_operands(M, N, K, 4000 + N + K, kinds=("e4m3", "e4m3") if fp8 else ("bf16", "bf16")))
        scale = FP8_DEQ[0] * FP8_DEQ[1] if fp8 else 1.0
        Av, Bv = (operand_values(A, "e4m3") * FP8_DEQ[0], operand_values(B, "e4m3") * FP8_DEQ[1]) if fp8 else (A, B)
        premise(Av, Bv, t.bias, t.res, unit=scale)
        pre = torch.full((M, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
        y = torch.zeros_like(pre)
        deq = torch.tensor(FP8_DEQ, dtype=torch.float32, device=DEV)
        p = t.params()
        p.A, p.B = A.data_ptr(), B.data_ptr()
        p.bias, p.res, p.ldr = t.bias.data_ptr(), t.res.data_ptr(), N
        p.C, p.ldc, p.C2, p.ldc2 = pre.data_ptr(), N, y.data_ptr(), N
        if fp8:
            p.deq_a, p.deq_b = deq.data_ptr(), deq.data_ptr() + 4
            assert L.plb_launch_gemm_nt_fp8_ln(C.byref(p), 5, 0, stream()) == 0
        else:
            assert L.plb_launch_gemm_nt_ln(C.byref(p), 5, stream()) == 0
        torch.cuda.synchronize()
        assert_exact(pre, rne_bf16(exact_nt(Av, Bv, t.bias, t.res)), 128, TN, f"LayerNorm form 5 {M}x{N}x{K} fp8 {fp8}: pre")
        assert int(t.err.item()) == 0 and int(t.xchg.abs().sum().item()) == 0


@pytest.mark.parametrize("ce_cols", CE_COLS)
@pytest.mark.parametrize("tile", CE_TILES)
def test_cross_entropy_pass_values(tile, ce_cols):
    """Pass 3 of the fused GEMM + cross-entropy: ce_tlogit is the target's logit and ce_pmax the per-tile row maximum over
    the real classes, bit for bit; a column tile without a real class (ce_cols 200: tile 1) reports -inf and a zero sum."""
    L = _lib.lib()
    M, N, K = CE_SHAPE
    A, B, bias, _ = dev(*nt_operands(M, N, K, 5000))
    premise(A, B, bias)
    logits = exact_nt(A, B, bias)
    tgt = torch.randint(0, ce_cols, (M,), generator=torch.Generator().manual_seed(ce_cols)).to(DEV)
    nt = N // 256
    pmax, psum = (torch.full((M, nt), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(2))
    tlogit = torch.full((M,), SENTINEL, dtype=torch.float32, device=DEV)
    p = _lib.PlbGemmNT()
    p.A, p.lda, p.B, p.ldb, p.M, p.N, p.K, p.Mstore = A.data_ptr(), K, B.data_ptr(), K, M, N, K, M
    p.bias, p.ce_cols, p.ce_tgt = bias.data_ptr(), ce_cols, tgt.data_ptr()
    p.ce_pmax, p.ce_psum, p.ce_tlogit = pmax.data_ptr(), psum.data_ptr(), tlogit.data_ptr()
    assert L.plb_launch_gemm_nt_big(C.byref(p), tile, 3, 0, stream()) == 0
    torch.cuda.synchronize()
    TM = 256 if tile == 256 else 128
    assert_exact(tlogit[:, None], logits.gather(1, tgt[:, None]), TM, 1, f"tile {tile} ce_cols {ce_cols}: ce_tlogit")
    real = logits.clone()
    real[:, ce_cols:] = float("-inf")
    assert_exact(pmax, real.reshape(M, nt, 256).amax(2), TM, 1, f"tile {tile} ce_cols {ce_cols}: ce_pmax (column = column tile)")
    for t in range(nt):
        if t * 256 >= ce_cols:
            assert bool((pmax[:, t] == float("-inf")).all()) and bool((psum[:, t] == 0).all()), f"empty column tile {t}"
        else:   # the maximum itself contributes exp(0) = 1
            assert bool((psum[:, t] >= 1.0).all()) and bool(torch.isfinite(psum[:, t]).all())


# ---- 3b gelu epilogues on exact pre-activations --------------------------------------------------------------------------------
def gelu_excess(g, u):
    """|g - gelu64(u)| as a fraction of the allowance: one bf16 spacing of the reference, floor 2^-64."""
    ref = gelu64(u)
    return (g.double() - ref).abs() / spacing_bf16(ref).clamp_min(2.0 ** -64)


def worst(excess, *named):
    i = tuple(int(v) for v in (excess == excess.max()).nonzero()[0])
    return f"{float(excess[i]):.4f} of the allowance at {list(i)}: " + ", ".join(f"{n} {float(t[i])!r}" for n, t in named)


@pytest.mark.parametrize("form", list(NT_FORMS))
def test_gelu_epilogues_on_exact_preactivations(form):
    TM, TN, (M, N), _ = NT_FORMS[form]
    A, B, bias, _ = dev(*nt_operands(M, N, 64 * GELU_KTILES, 7000 + form, b_unit=GELU_UNIT, bias_hi=2))
    premise(A, B, bias, unit=GELU_UNIT)
    # aux: every bf16 multiple of 1/8 in [-8, 8]
    aux = (int_operands((M, N), -64, 64, 7100 + form, "f32") / 8.0).to(torch.bfloat16).to(DEV)
    assert aux.float().unique().numel() == 129
    with forced(form):
        u, g = gemm_nt(A, B, N, bias=bias, act=1, fill=SENTINEL)
        du, _ = gemm_nt(A, B, N, aux=aux, act=2, fill=SENTINEL)
    assert_exact(u, rne_bf16(exact_nt(A, B, bias)), TM, TN, f"form {form} act 1: C = u")
    e1 = gelu_excess(g, u)
    v = exact_nt(A, B)
    ref = v * gelu_grad64(aux)
    e2 = (du.double() - ref).abs() / (spacing_bf16(ref) + v.abs() * 2.0 ** -16)
    r1, r2 = worst(e1, ("u", u), ("C2", g)), worst(e2, ("v", v), ("aux", aux), ("C", du), ("reference", ref))
    print(f"\ngelu form {form}: act 1 {r1} | act 2 {r2}")
    assert float(e1.max()) <= 1.0, f"form {form} act 1: {r1}"
    assert float(e2.max()) <= 1.0, f"form {form} act 2: {r2}"


# ---- 3c TN, bitwise -----------------------------------------------------------------------------------------------------------
def check_tn(kind, row, seed):
    Mtot, Ncols, N, K, splits, rps, lda, ldb = row
    fp8 = kind == "fp8"
    kinds = ("e5m2", "e4m3") if fp8 else ("bf16", "bf16")
    A, B = dev(*tn_operands(Mtot, Ncols, K, seed, kinds=kinds))
    scale = FP8_DEQ[0] * FP8_DEQ[1] if fp8 else 1.0
    Av, Bv = (operand_values(A, kinds[0]) * FP8_DEQ[0], operand_values(B, kinds[1]) * FP8_DEQ[1]) if fp8 else (A, B)
    premise(Av.T, Bv.T, unit=scale)
    As, _ = strided(A, lda, 0x3C if fp8 else 2.5)
    Bs, _ = strided(B, ldb, 0x3C if fp8 else -1.5)
    T = 128 if kind == "small" else 256
    what = f"TN {kind} {row}"
    buf = gemm_tn_slabs(As, Bs, N, splits, rps, kind, deq=FP8_DEQ, tail=(Ncols - N) * K)
    want = exact_tn(Av, Bv, N, splits, rps)
    slabs = buf[:splits * N * K].reshape(splits, N, K)
    for s in range(splits):   # splits == 1 is the direct form: the slab IS the output, every element written and exact
        assert_exact(slabs[s], want[s], T, T, f"{what}, slab {s}")
    assert_untouched(buf[splits * N * K:], f"{what}: rows >= N")
    if splits > 1:
        out = torch.full((N, K), SENTINEL, dtype=torch.float32, device=DEV)
        assert_exact(reduce_slabs(buf, splits, N * K, out, 0), want.sum(0), T, T, f"{what}, reduced")
        base = int_operands((N, K), -1000, 1000, seed + 7, "f32").to(DEV)
        out = base.clone()
        assert_exact(reduce_slabs(buf, splits, N * K, out, 1), want.sum(0) + base.double(), T, T, f"{what}, accumulated")


@pytest.mark.parametrize("case", range(len(TN_SMALL)))
def test_tn_small_bitwise(case):
    check_tn("small", TN_SMALL[case], 6000 + case)


@pytest.mark.parametrize("case", range(len(TN_BIG)))
def test_tn_big_bitwise(case):
    check_tn("big", TN_BIG[case], 6000 + len(TN_SMALL) + case)


@pytest.mark.parametrize("case", range(len(TN_FP8)))
def test_tn_fp8_bitwise(case):
    check_tn("fp8", TN_FP8[case], 6500 + case)


@pytest.mark.parametrize("case", range(len(TN_PLANNED)))
def test_tn_bitwise_on_the_plans_splits(case):
    """The same check with the splits the engine launches: kernel, splits and rows per split from plb_gemm_tn_plan."""
    kind, Mtot, Ncols, N, K, lda, ldb = TN_PLANNED[case]
    p = _lib.gemm_tn_plan(Mtot, Ncols, N, K, int(kind == "fp8"))
    assert (p["rc"], p["kernel"]) == (0, {"small": 0, "big": 1, "fp8": 2}[kind]), p
    assert (p["splits"], p["rows_per_split"]) == TN_PLANNED_SPLITS[case], p
    check_tn(kind, (Mtot, Ncols, N, K, p["splits"], p["rows_per_split"], lda, ldb), 6600 + case)


@pytest.mark.parametrize("splits", [3, 5])
def test_reduce_slabs_exact(splits):
    """Split counts that are no power of two, overwrite and accumulate: integer slabs sum exactly."""
    n = 4 * 257
    slab = int_operands((splits, n), -100000, 100000, 40 + splits, "f32").to(DEV)
    base = int_operands((n,), -100000, 100000, 50 + splits, "f32").to(DEV)
    out = torch.full((n,), SENTINEL, dtype=torch.float32, device=DEV)
    assert torch.equal(reduce_slabs(slab, splits, n, out, 0).double(), slab.double().sum(0))
    out = base.clone()
    assert torch.equal(reduce_slabs(slab, splits, n, out, 1).double(), slab.double().sum(0) + base.double())
