"""No GPU: the exact-arithmetic method of tests/test_gpu_gemm_exact.py checks itself on the CPU.

Premise. For every row of every case table the GPU module launches (gpu_util.exact_cases builds the operands as that module
does): the sum of the terms' magnitudes stays below 2^24 units (gpu_util.exact_bound), the values survive the cast to their
storage type (bf16, e4m3, e5m2), and an fp32 evaluation that walks the K-tiles of 64 in a shuffled order equals the float64
reference bit for bit — so any order a kernel sums in must give the same bits.

Checker. gpu_util.first_mismatch reports nothing on a clean evaluation and locates five simulated defects in the right
tile and 64x32 wave patch: one K-tile missing in one 16x16 patch; two B rows swapped; the residual read at row stride N
instead of ldr; the bias added twice in one column tile; one split of a TN sum counted twice.

Gelu allowances. gpu_util.gelu_f32_restatement (csrc/common.h gelu_new_f / gelu_new_grad_f in float32 numpy, same operation
order and constants) on EVERY bf16 value with |x| <= 16, against float64 in the cancellation-free form x / (1 + exp(-2z)):
    gelu, rounded to bf16:  at most 1 bf16 spacing of the reference (floor 2^-64)   measured 0.4998 of a spacing
    gelu'                :  at most 2^-16 absolute                                  measured 1.9e-06 (2^-16 = 1.5e-05)
(figures of this file's own run, printed with -s). At x = +16 and -16 the fp32 evaluation saturates: gelu' is exactly 1 and
exactly 0 there, which is what lets the GPU module hold the act 2 launches with column-sum partials bit for bit.
"""
import numpy as np
import pytest
import torch

from gpu_util import (EXACT_LIMIT, GELU_UNIT, exact_bound, exact_cases, exact_nt, exact_tn, first_mismatch, gelu64, gelu_f32_restatement,
                      gelu_grad64, int_operands, mismatch_location, nt_operands, operand_values, rne_bf16, spacing_bf16,
                      tn_operands)


def shuffled_f32(A, B, seed):
    """A.B^T accumulated in fp32, K-tile by K-tile (64 columns) in a shuffled order."""
    K = A.shape[1]
    order = torch.randperm((K + 63) // 64, generator=torch.Generator().manual_seed(seed))
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float32)
    for t in order.tolist():
        acc += A[:, 64 * t:64 * t + 64].float() @ B[:, 64 * t:64 * t + 64].float().T
    return acc


def test_premise_holds_for_every_table_row():
    worst = 0.0
    n = 0
    for name, A, B, bias, res, unit in exact_cases():
        bound = exact_bound(A, B, bias, res, unit)
        assert bound < EXACT_LIMIT, (name, bound)
        worst = max(worst, bound)
        n += 1
        K = A.shape[1]
        if name.startswith("nt") and unit == 1.0:       # the NT tables' own promise: <= 16 K + 192
            assert bound <= 16 * K + 192, (name, bound)
        # any summation order gives the same fp32 bits (checked where it costs little: K up to 7 tiles, and the longest)
        if K <= 448 or K >= 2112:
            ref = exact_nt(A, B)
            assert torch.equal(shuffled_f32(A, B, seed=n).double(), ref), name
    print(f"\npremise: {n} cases, largest sum of magnitudes {worst:.0f} units of 2^24 = {EXACT_LIMIT:.0f}")


@pytest.mark.parametrize("kind", ["bf16", "e4m3", "e5m2"])
def test_values_survive_the_cast_to_their_storage_type(kind):
    x = int_operands((64, 64), -4, 4, 1, kind)
    want = int_operands((64, 64), -4, 4, 1, "f32")
    assert torch.equal(operand_values(x, kind), want.double())
    assert set(want.flatten().tolist()) == set(float(v) for v in range(-4, 5))
    if kind == "bf16":   # the gelu cases' power-of-two factor, the bias and the residual ranges
        assert torch.equal(int_operands((64, 64), -4, 4, 2, "bf16", GELU_UNIT).double(), int_operands((64, 64), -4, 4, 2, "f32").double() * GELU_UNIT)
        r = torch.arange(-128, 129).float()
        assert torch.equal(r.to(torch.bfloat16).float(), r)


# ---- the checker ----------------------------------------------------------------------------------------------------------
M, N, K, TM, TN, LDR = 384, 768, 192, 128, 256, 776


@pytest.fixture(scope="module")
def clean():
    A, B, bias, res = nt_operands(M, N, K, 77)
    return A, B, bias, res, exact_nt(A, B, bias, res)


def test_clean_evaluation_has_no_mismatch(clean):
    A, B, bias, res, ref = clean
    got = shuffled_f32(A, B, 5) + bias + res.float()
    assert first_mismatch(got, ref, TM, TN) is None
    assert first_mismatch(got.to(torch.bfloat16), rne_bf16(ref), TM, TN) is None


def test_missing_k_tile_in_one_patch_is_located(clean):
    A, B, bias, res, ref = clean
    r0, c0, kt = 128 + 64 + 16, 256 + 3 * 32 + 16, 1
    bad = ref.clone()
    bad[r0:r0 + 16, c0:c0 + 16] -= A[r0:r0 + 16, 64 * kt:64 * kt + 64].double() @ B[c0:c0 + 16, 64 * kt:64 * kt + 64].double().T
    for got, want in ((bad.float(), ref), (rne_bf16(bad), rne_bf16(ref))):
        count, rt, ct, patch = mismatch_location(got, want, TM, TN)
        assert (rt, ct, patch) == (1, 1, (1, 3)) and 200 <= count <= 256, (count, rt, ct, patch)
    msg = first_mismatch(bad.float(), ref, TM, TN)
    assert "row tile 1, column tile 1, wave patch (1, 3)" in msg, msg


def test_swapped_b_rows_are_located(clean):
    A, B, bias, res, ref = clean
    j1, j2 = 300, 301
    Bs = B.clone()
    Bs[[j1, j2]] = B[[j2, j1]]
    count, rt, ct, patch = mismatch_location(exact_nt(A, Bs, bias, res), ref, TM, TN)
    assert (ct, patch[1]) == (j1 // TN, j1 % TN // 32) and rt == 0 and M <= count <= 2 * M, (count, rt, ct, patch)


def test_residual_read_at_the_wrong_row_stride_is_located(clean):
    A, B, bias, res, ref = clean
    buf = torch.full((M, LDR), 99.0, dtype=torch.bfloat16)
    buf[:, :N] = res
    wrong = buf.flatten()[:M * N].reshape(M, N)                      # row m read at m * N instead of m * LDR
    got = exact_nt(A, B, bias, wrong)
    count, rt, ct, patch = mismatch_location(got, ref, TM, TN)
    assert torch.equal(got[0], ref[0]) and (rt, patch[0]) == (0, 0) and count > (M - 1) * N // 2, (count, rt, ct, patch)
    assert "first at (1, " in first_mismatch(got, ref, TM, TN)


def test_bias_added_twice_in_one_column_tile_is_located(clean):
    A, B, bias, res, ref = clean
    got = ref.clone()
    got[:, TN:2 * TN] += bias[TN:2 * TN].double()
    count, rt, ct, patch = mismatch_location(got, ref, TM, TN)
    first = int((bias[TN:2 * TN] != 0).nonzero()[0])
    assert (rt, ct, patch) == (0, 1, (0, first // 32)) and count == M * int((bias[TN:2 * TN] != 0).sum()), (count, rt, ct, patch)


def test_split_counted_twice_is_located():
    Mtot, Ncols, Kc, splits, rps = 320, 256, 256, 3, 128
    A, B = tn_operands(Mtot, Ncols, Kc, 78)
    slabs = exact_tn(A, B, Ncols, splits, rps)
    ref = A.double().T @ B.double()
    assert first_mismatch(slabs.sum(0).float(), ref, 256, 256) is None
    got = slabs.sum(0) + slabs[1]
    count, rt, ct, patch = mismatch_location(got.float(), ref, 256, 256)
    r, c = (int(v) for v in (slabs[1] != 0).nonzero()[0])
    assert count == int((slabs[1] != 0).sum()) and (rt, ct, patch) == (0, 0, (r // 64, c // 32)), (count, rt, ct, patch)


# ---- the gelu allowances ----------------------------------------------------------------------------------------------------
def test_gelu_restatement_is_inside_both_allowances():
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.bfloat16).float()
    x = x[torch.isfinite(x) & (x.abs() <= 16)]
    assert x.numel() > 33000                                                   # every bf16 value in range, both signs
    g32, d32 = gelu_f32_restatement(x.numpy())
    g = torch.from_numpy(g32).to(torch.bfloat16).double()                      # as the kernel stores it
    ref = gelu64(x)
    ratio = (g - ref).abs() / torch.maximum(spacing_bf16(ref), torch.tensor(2.0 ** -64, dtype=torch.float64))
    derr = (torch.from_numpy(d32).double() - gelu_grad64(x)).abs()
    print(f"\ngelu: at most {float(ratio.max()):.4f} of a bf16 spacing (x = {float(x[ratio.argmax()])!r}); "
          f"gelu': at most {float(derr.max()):.2e} absolute (x = {float(x[derr.argmax()])!r})")
    assert float(ratio.max()) <= 1.0
    assert float(derr.max()) <= 2.0 ** -16
    # the naive float64 form is NOT a reference: it cancels to 0 below -7.2
    naive = 0.5 * x.double() * (1.0 + torch.tanh(0.7978845608028654 * (x.double() + 0.044715 * x.double() ** 3)))
    assert bool((naive[x < -9] == 0).all()) and bool((ref[x < -9] < 0).all())
    # saturation at +-16: the derivative is exactly 1 / exactly 0 (the act 2 + colpart launches rely on it)
    _, d = gelu_f32_restatement(np.array([16.0, -16.0], dtype=np.float32))
    assert d[0] == 1.0 and d[1] == 0.0
