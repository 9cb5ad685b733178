"""-m gpu: the gradient buffer of one training call, SLICE BY SLICE against float64 (tests/grad_slices_ref.py holds the contract).

What is under test is not a kernel (those have their own per-element modules) but the launch sequences of
csrc/engine_layers.cpp and csrc/engine_calls.cpp that turn the kernels into a gradient buffer: the per-layer slots, the
weight-gradient GEMMs over the stacked rows of the L applications with their split rule and slab reduction, the colpart /
ducol / qkvcol partial rows finished into bias gradients, the LayerNorm partials summed over the applications, the pruned
last application with its scatter back to token rows, the packed row plans, the fused and the unfused forms. The per-tensor
relative L2 of 4e-2 the engine tests allow cannot see a fault confined to one row, one column or one bias block
(tests/test_grad_slices_host.py shows six that it passes); here every row and column of every 2-D gradient and every
64-element block of every 1-D gradient is held to the float64 oracle within FACTOR x the slice's scale, where the scale is
the largest error of four bf16 restatements of the step on that slice (floored at the median over the tensor's slices) and
FACTOR = 2 x loo, the restatements' own leave-one-out spread. Slices whose reference is exactly zero (absent word ids and
row 0, position rows at or past S, the unused token-type row) must be exactly zero, and as many of them as the reference
has. The key bias (true gradient zero) keeps its norm rule. Loss within 1e-3, no LayerNorm hand-off timeout, and the
launch classes each case is there for are counted (profile hooks) so that a case cannot silently stop reaching its form.

One fresh engine and one loss_fwd_bwd per parameter; the reference of a case is built once (2 s small, 9 s h768, 14 s h512 on
the CPU) and shared by its modes.

Cases (the smallest shapes that reach each form) and their bound — computed on the CPU, nothing from the device:

    case    model (E / H / heads / FFN / L)   batch                                    Tp      loo     FACTOR
    small   64 / 128 / 2 / 256 / 3            5 x 90, lengths 90 77 64 13 1            512     1.119   2.239
    h512    128 / 512 / 8 / 1024 / 4          8 x 256, two samples cut to 120 and 37   2048    2.926   5.852
    h768    128 / 768 / 12 / 2048 / 2         4 x 256, one sample cut to 100           1024    1.956   3.912

  small  unfused LayerNorm kernels, 128x128 GEMM tiles for everything but the FFN pair (512 rows x 256: the gelu-derivative
         stash on one 256x256 tile row pair), 128x128 weight-gradient kernel, a sample with ONE key, S no multiple of 32.
  h512   fused LayerNorm epilogues on 256-column tiles with the two-tile exchange, the gelu-derivative stash, 8192 stacked
         rows: the 256x256 weight-gradient kernel with row splits and slab reduction for Q/K/V (and for all four with
         pruning off; pruned, the other three stack 6144 + Mc rows and take the 128x128 kernel), the small TN kernel for
         the E -> H mapping, the pruned last application.
  h768   the production 128x384 LayerNorm tile form, pruning.

Modes: default | pruning off (plb_set_prune_last(0)) | LayerNorm fusion off (PLBERT_LN_FUSE=off) | token-packed
(packing_plan) | attention backward forced to the two-kernel form | to the single-kernel form.

Worst err / scale per case and mode over all tensors, and the tensor it sits in, measured on an MI355X (a record; the bound
does not come from these):

    case-mode          worst err / scale   FACTOR   where
    small-default      1.129               2.239    token_type_embeddings.weight, col 37
    small-noprune      1.123               2.239    ffn_output.bias, block 0
    small-lnoff        -                            (skipped: no fused form at this shape)
    small-packed       -                            (skipped: five slots of 128 rows are no fewer than 5 x 90 padded to 512)
    small-attn-split   1.129               2.239    token_type_embeddings.weight, col 37
    small-attn-fused   1.129               2.239    token_type_embeddings.weight, col 37
    h512-default       2.417               5.852    attention.dense.weight, row 273
    h512-noprune       2.449               5.852    embedding_hidden_mapping_in.weight, row 454
    h512-lnoff         2.286               5.852    position_embeddings.weight, col 79
    h512-packed        2.286               5.852    position_embeddings.weight, col 79   (1792 rows: unfused, as lnoff)
    h512-attn-split    2.417               5.852    attention.dense.weight, row 273
    h512-attn-fused    2.394               5.852    attention.dense.weight, row 273
    h768-default       2.492               3.912    attention.query.weight, row 342
    h768-noprune       2.346               3.912    attention.query.weight, row 342
    h768-lnoff         2.767               3.912    attention.query.weight, row 342
    h768-packed        2.626               3.912    attention.query.weight, row 342     (896 rows: unfused, no gelu stash)
    h768-attn-split    2.492               3.912    attention.query.weight, row 342
    h768-attn-fused    2.492               3.912    attention.query.weight, row 342

The device sits about where the restatements sit among themselves (loo 1.12 / 2.93 / 1.96): at 0.4 to 0.5 of FACTOR in the
small and h512 cases, at 0.60 to 0.71 of it in h768. -s prints every tensor's worst slice per case and mode.

What the bound resolves, from one experiment on the device (a build, not kept, whose column sums of the Q/K/V bias partial
rows and of the LayerNorm-1 partial rows each skipped their first row): 14 of the 16 parameters failed — value.bias at 10 x
its scale in small, dense.bias at 7.4 x in h512 and 42 x in h768, where the per-tensor figures of test_gpu_engine.py were
4.3e-2 to 7.2e-2 against their 4e-2. h512-lnoff and h512-packed passed: there one of 2048 partial rows is 4 of 8192 token
rows, an estimated (4 / 8192)^0.5 = 2e-2 of the bias gradient spread evenly over its blocks, which is inside FACTOR x the bf16 noise of every block. A
fault has to stand clear of the rounding noise OF ITS SLICE to be seen; spread thinly over a whole tensor it is not.
"""
import numpy as np
import pytest
import torch

import grad_slices_ref as R
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import HipEngine, packing_plan

pytestmark = pytest.mark.gpu

MODES = ("default", "noprune", "lnoff", "packed", "attn-split", "attn-fused")


def _params():
    out = []
    for case in R.CASES:
        for mode in MODES:
            marks = []
            if mode == "lnoff" and case == "small":
                marks = [pytest.mark.skip(reason="H = 128 / 512 rows has no fused LayerNorm form to turn off: the default mode is this run")]
            out.append(pytest.param(case, mode, marks=marks, id=f"{case}-{mode}"))
    return out


def _fusable(H, Tp):
    """csrc/engine_layers.cpp ln_fusable: 1024-row multiples, at most four column tiles of 384 or 256."""
    return Tp % 1024 == 0 and (H // 384 if H % 384 == 0 else H // 256 if H % 256 == 0 else 99) <= 4


@pytest.mark.parametrize("name,mode", _params())
def test_gradient_slices(name, mode, monkeypatch):
    c = R.build_case(name)
    spec, cfg = c["spec"], c["spec"]["cfg"]
    B, S, L, H, I = spec["B"], spec["S"], cfg["num_hidden_layers"], cfg["hidden_size"], cfg["intermediate_size"]
    lib = _lib.lib()
    lens = np.asarray(c["lengths"], np.int32)
    off, flat = plbert_amd.masked_indices_to_csr(c["idx"])
    plan = None
    if mode == "packed":
        plan = packing_plan(c["lengths"], S)
        if not plan.packed:
            pytest.skip("the plan of these lengths is the padded layout itself (128-row slots save nothing): the call would run padded")
    if mode == "lnoff":
        monkeypatch.setenv("PLBERT_LN_FUSE", "off")      # read when the engine is created
    try:
        if mode == "noprune":
            lib.plb_set_prune_last(0)
        if mode.startswith("attn-"):
            lib.plb_set_attn_bwd_fused(1 if mode == "attn-fused" else 0)
        eng = HipEngine(c["pcfg"], 188, 0, max_batch=B, max_seq=S)
        eng.load_state_dict(c["sd"])
        _lib.profile_enable(True)
        try:
            loss = eng.loss_fwd_bwd(c["masked"], c["labels"], lens, off, flat, int(off[-1]), packing=plan)
            torch.cuda.synchronize()
            prof = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
    finally:
        lib.plb_set_prune_last(-1)
        lib.plb_set_attn_bwd_fused(-1)
    n = lambda cls: prof.get(cls, {}).get("launches", 0)
    counts = {k: n(k) for k in ("gemm_nt_lnfwd", "gemm_nt_lnbwd", "gemm_nt_gelu", "gemm_nt_gelubwd", "gemm_tn", "reduce_slabs",
                                "attn_bwd", "attn_bwd_dq", "attn_bwd_dkv", "gather_scatter_rows", "ln_fwd", "ln_bwd")}
    rows, of = eng.last_application_rows()
    ran, stood_for = eng.last_call_rows()
    Tp = -(-ran // 128) * 128
    print(f"\nslices {name}-{mode}: loss {float(loss.item()):.6f} (oracle {c['loss']:.6f}), rows {ran} of {stood_for}, last application "
          f"on {rows} of {of}, launches {counts}")

    # ---- the contract ----
    assert abs(float(loss.item()) - c["loss"]) / c["loss"] < 1e-3, (float(loss.item()), c["loss"])
    assert eng.status()["ln_exchange_timeouts"] == 0
    got = {k: eng.view(k, of=eng.grads).double().cpu().numpy() for k in c["ref"]}
    try:
        stats = R.check_slices(c, got)
    except AssertionError:
        try:   # the whole picture before the first violation is raised: every tensor's worst slice, at a bound nothing exceeds
            R.report(f"{name}-{mode} (FAILS at FACTOR {c['factor']:.3f})", R.check_slices(c, got, factor=np.inf))
        except AssertionError:
            pass   # (a zero rule: no ratio to report)
        raise
    R.report(f"{name}-{mode}", stats)
    worst = max(stats.items(), key=lambda kv: kv[1]["ratio"])
    print(f"slices {name}-{mode}: WORST {worst[1]['ratio']:.3f} of FACTOR {c['factor']:.3f} in {worst[0]} ({worst[1]['axis']} {worst[1]['slice']})")
    assert {k: s["zeros"] for k, s in stats.items()} == c["zeros"]

    # ---- the forms the case is there for really ran ----
    pruned = mode != "noprune"
    assert (rows < of) == pruned and rows % 128 == 0, (rows, of)
    assert (ran < stood_for) == (mode == "packed"), (ran, stood_for)
    full = L - 1 if pruned else L                          # applications whose post-attention part runs on all rows
    fused = mode != "lnoff" and _fusable(H, Tp)
    assert fused == (name != "small" and mode not in ("lnoff", "packed")), (name, mode, Tp)
    # fused: dense + LayerNorm 1 and FFN output + LayerNorm 2 forward per full application; backward, LayerNorm 1 per full
    # application and LayerNorm 2 of every application but the last (whose output gradient comes from the head)
    assert counts["gemm_nt_lnfwd"] == (2 * full if fused else 0) and counts["gemm_nt_lnbwd"] == (full + L - 1 if fused else 0), counts
    assert (counts["ln_fwd"] > 2) == (not fused), counts   # (the embeddings and a pruned last application use the kernel anyway)
    if Tp % 256 == 0 and I % 256 == 0:                     # the gelu-derivative stash pair, per full application
        assert counts["gemm_nt_gelu"] == full and counts["gemm_nt_gelubwd"] == full, counts
    single = mode == "attn-fused"
    assert counts["attn_bwd"] == (L if single else 0) and counts["attn_bwd_dq"] == counts["attn_bwd_dkv"] == (0 if single else L), counts
    # weight gradients: head, map-in, Q/K/V, ffn, ffn_output, dense; 8192 stacked rows put Q/K/V on the 256x256 kernel
    assert counts["gemm_tn"] == 6 and counts["reduce_slabs"] >= 4, counts
    if name == "h512" and mode != "packed":
        assert L * Tp == 8192 and (L - 1) * Tp + rows == (8192 if mode == "noprune" else 6144 + rows)


def test_device_gradients_with_a_defect_fail():
    """The defects of tests/test_grad_slices_host.py laid over the DEVICE's gradients of the small case instead of the
    stand-in's: each stays under the per-tensor 4e-2 and each is raised and named. (The device's own error is part of every
    slice here, so this is the check that the margin FACTOR leaves is not what hides a fault.)"""
    import re
    c = R.build_case("small")
    eng = HipEngine(c["pcfg"], 188, 0, max_batch=c["spec"]["B"], max_seq=c["spec"]["S"])
    eng.load_state_dict(c["sd"])
    off, flat = plbert_amd.masked_indices_to_csr(c["idx"])
    eng.loss_fwd_bwd(c["masked"], c["labels"], np.asarray(c["lengths"], np.int32), off, flat, int(off[-1]))
    torch.cuda.synchronize()
    clean = {k: eng.view(k, of=eng.grads).double().cpu().numpy() for k in c["ref"]}
    R.check_slices(c, clean)
    for what, inject, whole in R.DEFECTS:
        G = {k: g.copy() for k, g in clean.items()}
        tensor, axis, i = inject(c, G)
        per_tensor = R.rel_l2(G[tensor], c["ref"][tensor])
        ratio = R.slice_errors(G, c["ref"])[tensor, axis][i] / c["scale"][tensor, axis][i]
        print(f"\ndevice + {what}: {axis} {i}, per-tensor rel L2 {per_tensor:.3e}, err / scale {ratio:.1f}")
        assert per_tensor < R.PER_TENSOR, (what, per_tensor)
        with pytest.raises(AssertionError, match=re.escape(f"{tensor}: {axis} {i} is off by")):
            R.check_slices(c, G)
        if whole:
            assert ratio >= 1.5 * c["factor"], (what, ratio)
