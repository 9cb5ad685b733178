"""The kernels write what the plan says (-m gpu; csrc/gemm_nt_plan.cpp): for every NT GEMM form that leaves column-sum partials,
the launch overwrites exactly the plan's colpart_rows rows of a sentinel-filled buffer, leaves the rows behind them alone,
and the rows sum to the column sums of the output as stored (the tolerance of tests/test_gpu_kernels.py for colpart). The
engine sizes and indexes o_ducol / o_part1 / o_part2 / o_tcolp by the same number. One engine case holds the per-class launch
counts of a training step, fused (Tp = 1024) and unfused on the small kernel (Tp = 384), to those of the commit before the
plan unit (profiles/nt_plan_ab.txt)."""
import ctypes as C

import pytest
import torch

import plbert_amd
from gpu_util import SENTINEL, Ln, rel_l2, stream
from plbert_amd import _lib
from plbert_amd.engine import HipEngine
from test_gemm_nt_plan_host import (BF16, CE2, COLPART, E4M3, E5M2, GELUBWD, GELUD, GELUDBWD, LNBWD, PLAIN, plan)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4


def randbf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


def fp8_image(x, bf8):
    return x.float().to(torch.float8_e5m2 if bf8 else torch.float8_e4m3fn).view(torch.uint8)


def colpart_buffer(rows, width):
    return torch.full((rows + GUARD, width), SENTINEL, dtype=torch.float32, device=DEV)


def check_colpart(colp, rows, want_sums, what, pick=None):
    """colp [rows + GUARD, width]: every one of the plan's rows overwritten, the guard rows behind them untouched, and the
    rows (pick: the third of three blocks of a LayerNorm-backward row) sum to the column sums of the stored output."""
    torch.cuda.synchronize()
    assert rows > 0, what
    assert bool((colp[:rows] != SENTINEL).all()), f"{what}: {int((colp[:rows] == SENTINEL).sum())} elements of the plan's {rows} rows not written"
    assert bool((colp[rows:] == SENTINEL).all()), f"{what}: rows behind the plan's {rows} were written"
    part = colp[:rows] if pick is None else colp[:rows].view(rows, 3, -1)[:, pick]
    assert rel_l2(part.double().sum(0), want_sums.double()) < 1e-5, what


def desc(A, B, M, N, K):
    p = _lib.PlbGemmNT()
    p.A, p.lda, p.B, p.ldb, p.M, p.N, p.K, p.Mstore = A.data_ptr(), K, B.data_ptr(), K, M, N, K, M
    return p


def stash_rows(blob, M, N, tm):
    """The gelu'(u) stash of forms 7 / 8 from its LANE layout (csrc/gemm_nt_pipeline.h) to rows: per tm x 256 tile t (row-major
    tile order), slab (mh, mi) and column half nh, 512 consecutive 16-byte items, one per thread = {ni 0, ni 1} x 4 columns."""
    nbn = N // 256
    ar = lambda n, pos: torch.arange(n, device=blob.device).view(*[-1 if i == pos else 1 for i in range(7)])   # noqa: E731
    t, mh, mi, nh, tid, ni, r = ar((M // tm) * nbn, 0), ar(tm // 128, 1), ar(4, 2), ar(2, 3), ar(512, 4), ar(2, 5), ar(4, 6)
    uw, lane = tid >> 6, tid & 63
    wm, wn, frow, fq = uw >> 2, uw & 3, lane & 15, lane >> 4
    row = (t // nbn) * tm + mh * 128 + wm * 64 + mi * 16 + frow
    col = (t % nbn) * 256 + nh * 128 + wn * 32 + ni * 16 + fq * 4 + r
    out = torch.empty(M, N, dtype=blob.dtype, device=blob.device)
    row, col = torch.broadcast_tensors(row, col)
    out[row.reshape(-1), col.reshape(-1)] = blob.reshape(-1)
    return out


@pytest.fixture
def forced_tile():
    L = _lib.lib()
    yield L.plb_set_gemm_nt_tile
    L.plb_set_gemm_nt_tile(0)


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("tile,M,N", [(256, 512, 256), (384, 256, 384), (1256, 256, 768)])
def test_plain_and_gelu_backward_on_the_pipeline_kernel(forced_tile, act, tile, M, N):
    """plb_launch_gemm_nt with colpart: the smallest shapes go to the small kernel (colpart refused: 1) unless the tile hook
    names a pipeline tile."""
    L, K = _lib.lib(), 64
    A, B, u = randbf(M, K, seed=1), randbf(N, K, scale=0.2, seed=2), randbf(M, N, seed=3)
    out = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    p = desc(A, B, M, N, K)
    p.C, p.ldc = out.data_ptr(), N
    if act == 2:
        p.aux, p.ldaux = u.data_ptr(), N
    form = GELUBWD if act == 2 else PLAIN
    assert plan(L, M, N, K, form, BF16, COLPART)["rc"] == 1
    p.colpart = colpart_buffer(1, N).data_ptr()
    assert L.plb_launch_gemm_nt(C.byref(p), act, 0, stream()) == 1
    forced_tile(tile)
    pl = plan(L, M, N, K, form, BF16, COLPART)
    assert pl["rc"] == 0 and pl["tile"] == tile
    colp = colpart_buffer(pl["colpart_rows"], N)
    p.colpart = colp.data_ptr()
    assert L.plb_launch_gemm_nt(C.byref(p), act, 0, stream()) == 0
    check_colpart(colp, pl["colpart_rows"], out.double().sum(0), (act, tile))


@pytest.mark.parametrize("tile,M", [(256, 512), (1256, 384)])
def test_cross_entropy_pass_2(forced_tile, tile, M):
    L, N, K = _lib.lib(), 256, 64
    A, B = randbf(M, K, seed=4), randbf(N, K, scale=0.2, seed=5)
    tgt = torch.randint(0, 200, (M,), device=DEV)
    lse, w = torch.full((M,), 3.0, device=DEV), torch.rand(M, device=DEV)
    dl = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    pl = plan(L, M, N, K, CE2, BF16, COLPART, tile)
    assert pl["rc"] == 0 and pl == plan(L, M, N, K, CE2, BF16, COLPART)      # the token head's tile at this M is this tile
    colp = colpart_buffer(pl["colpart_rows"], N)
    p = desc(A, B, M, N, K)
    p.ce_cols, p.ce_tgt, p.ce_lse, p.ce_w = 200, tgt.data_ptr(), lse.data_ptr(), w.data_ptr()
    p.C, p.ldc, p.colpart = dl.data_ptr(), N, colp.data_ptr()
    assert L.plb_launch_gemm_nt_big(C.byref(p), tile, 4, 0, stream()) == 0
    check_colpart(colp, pl["colpart_rows"], dl.double().sum(0), tile)
    # through plb_launch_gemm_nt the pass takes the tile of the per-shape policy: none at this size (small kernel: 1), the
    # forced one otherwise, with the same result
    first = dl.clone()
    assert L.plb_launch_gemm_nt(C.byref(p), 4, 0, stream()) == 1
    forced_tile(tile)
    dl.zero_()
    assert L.plb_launch_gemm_nt(C.byref(p), 4, 0, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dl, first)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("N", [256, 768])
def test_layernorm_backward(N, fp8):
    L, M, K = _lib.lib(), 1024, (128 if fp8 else 64)
    t = Ln(M, N, K, seed=N)
    pre = randbf(M, N, seed=77)
    x = pre.float()
    t.mean.copy_(x.mean(1)); t.rstd.copy_((x.var(1, unbiased=False) + 1e-12).rsqrt())
    dx = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    pl = plan(L, M, N, K, LNBWD, E5M2 if fp8 else BF16, 0)
    assert pl["rc"] == 0
    colp = colpart_buffer(pl["colpart_rows"], 3 * N)
    p = t.params()
    p.res, p.ldr, p.aux, p.ldaux = t.res.data_ptr(), N, pre.data_ptr(), N
    p.C, p.ldc, p.colpart = dx.data_ptr(), N, colp.data_ptr()
    if fp8:
        A8, B8, deq = fp8_image(t.A, True), fp8_image(t.B * 8, False), torch.tensor([1.0, 0.125], device=DEV)
        p.A, p.B, p.deq_a, p.deq_b = A8.data_ptr(), B8.data_ptr(), deq.data_ptr(), deq.data_ptr() + 4
        assert L.plb_launch_gemm_nt_fp8_ln(C.byref(p), 6, 1, stream()) == 0
    else:
        assert L.plb_launch_gemm_nt_ln(C.byref(p), 6, stream()) == 0
    check_colpart(colp, pl["colpart_rows"], dx.double().sum(0), (N, fp8), pick=2)
    assert int(t.err.item()) == 0


@pytest.mark.parametrize("fp8,M", [(False, 256), (False, 512), (True, 256), (True, 128)])
def test_derivative_stash_forward_and_backward(fp8, M):
    """Forward with colpart (the column sums of the stashed derivative as stored) and backward (of dU), at both row-tile
    heights of the fp8 launcher."""
    L, N, K = _lib.lib(), 256, (128 if fp8 else 64)
    A, B = randbf(M, K, seed=6), randbf(N, K, scale=0.15, seed=7)
    A2 = randbf(M, K, seed=8)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(9)) * 0.1).to(DEV)
    stash, gelu, du = (torch.zeros(M, N, dtype=torch.bfloat16, device=DEV) for _ in range(3))
    deq = torch.tensor([1.0, 0.125], device=DEV)
    B8 = fp8_image(B * 8, False)

    def launch(bwd, operand, colp):
        a_op = fp8_image(operand, bwd) if fp8 else operand
        p = desc(a_op, B8 if fp8 else B, M, N, K)
        p.colpart = colp.data_ptr()
        if bwd:
            p.aux, p.ldaux, p.C, p.ldc = stash.data_ptr(), N, du.data_ptr(), N
        else:
            p.bias, p.C, p.ldc, p.C2, p.ldc2 = bias.data_ptr(), stash.data_ptr(), N, gelu.data_ptr(), N
        if fp8:
            p.deq_a, p.deq_b = deq.data_ptr(), deq.data_ptr() + 4
            return L.plb_launch_gemm_nt_fp8_gelud(C.byref(p), int(bwd), int(bwd), stream())
        return L.plb_launch_gemm_nt_gelud(C.byref(p), int(bwd), stream())

    fwd = plan(L, M, N, K, GELUD, E4M3 if fp8 else BF16, COLPART)
    bwd = plan(L, M, N, K, GELUDBWD, E5M2 if fp8 else BF16, COLPART)
    assert fwd["rc"] == 0 and bwd["rc"] == 0 and fwd["tile_m"] == bwd["tile_m"] == (128 if M == 128 else 256)
    if fp8:
        assert L.plb_gemm_nt_fp8_gelud_tile_rows(M) == fwd["tile_m"]
    colp = colpart_buffer(fwd["colpart_rows"], N)
    assert launch(False, A, colp) == 0
    check_colpart(colp, fwd["colpart_rows"], stash_rows(stash, M, N, fwd["tile_m"]).double().sum(0), ("forward", fp8, M))
    colp = colpart_buffer(bwd["colpart_rows"], N)
    assert launch(True, A2, colp) == 0
    check_colpart(colp, bwd["colpart_rows"], du.double().sum(0), ("backward", fp8, M))


# Launches per class of one bf16 loss_fwd_bwd with the profiler on, 2 applications of H = 256 / I = 512, pruned last
# application, measured on the commit BEFORE the plan unit (profiles/nt_plan_ab.txt, "launch counts"):
#   8 x 128 = 1024 rows: the fused LayerNorm and derivative-stash forms; 3 x 128 = 384 rows: no fused form, small kernel
PARENT_LAUNCHES = {
    1024: {"gemm_nt_f32": 1, "gemm_nt_gelu": 1, "gemm_nt_gelubwd": 1, "gemm_nt_lnbwd": 2, "gemm_nt_lnfwd": 2, "gemm_nt_small": 13, "gemm_tn": 6},
    384: {"gemm_nt_f32": 1, "gemm_nt_small": 19, "gemm_tn": 6},
}


def step_launches(B, S=128):
    pcfg = plbert_amd.AlbertConfig(vocab_size=188, embedding_size=128, hidden_size=256, num_attention_heads=4, intermediate_size=512,
                                   max_position_embeddings=512, num_hidden_layers=2)
    labels, masked, _, idx = plbert_amd.synthetic_batch(B, S, seed=7)
    eng = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(pcfg, 188, seed=3))
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    _lib.profile_enable(True)
    try:
        _lib.profile_read()
        loss = eng.loss_fwd_bwd(masked, labels, None, off, flat, int(off[-1]))
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    assert bool(torch.isfinite(loss).all())
    return {k: v["launches"] for k, v in sorted(prof.items()) if k.startswith("gemm_")}


@pytest.mark.parametrize("B", [8, 3])
def test_a_training_step_takes_the_launches_it_took(B):
    got = step_launches(B)
    print(f"launches at {B * 128} rows: {got}")
    assert got == PARENT_LAUNCHES[B * 128]
