"""The 64x64 form of the small NT GEMM kernel (-m gpu): the same launch in the 128x128 form (plb_set_gemm_nt_tile(-64))
and in the 64x64 form (64) on the same buffers must leave the same BYTES in every output. An output element depends on
the order in which its K-chunks of 32 enter the MFMA and on the epilogue applied to it, not on the tile it sits in: the
two forms share the fragment layout, the K order and nt_epilogue. Both are also held to a float64 product of the same
bf16 operands, within the tolerances tests/test_gpu_kernels.py uses for this kernel. Engine level: one training call per
form, loss and gradients equal bit for bit."""
import numpy as np
import pytest
import torch

import plbert_amd
from conftest import golden_cfg, load_golden
from gpu_util import SENTINEL, gelu64, gelu_grad64, gemm_nt, rel_l2
from plbert_amd import _lib
from plbert_amd.engine import HipEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def randbf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


def wide(t, extra):
    """t as a column slice of a buffer `extra` elements wider: a strided operand."""
    w = torch.zeros((t.shape[0], t.shape[1] + extra), dtype=t.dtype, device=t.device)
    w[:, : t.shape[1]] = t
    return w[:, : t.shape[1]]


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# name: (M, N, K, epilogue, options). Epilogues: "plain", "bias_res", "gelu" (ACT 1: u and gelu(u)), "gelu_bwd" (ACT 2 with
# aux), "f32" (the head's form: fp32 output with bias). Options: Mstore; strides = every leading dimension wider than its
# rows; ldcf. 64-form grids: 2 to 128 workgroups.
CASES = {
    "one_k_tile": (128, 128, 64, "plain", {}),
    "both_lds_stages": (128, 128, 128, "plain", {}),
    "odd_k_tile_count": (128, 128, 192, "bias_res", {}),
    "one_column_tile": (128, 64, 128, "plain", {}),
    "third_column_tile_of_4": (128, 132, 128, "bias_res", {}),        # n0 >= N inside the last 64-column tile
    "four_columns": (128, 4, 128, "bias_res", {}),
    "row_guard_inside_a_tile": (256, 128, 128, "bias_res", {"Mstore": 130}),
    "strides": (128, 192, 192, "bias_res", {"strides": True}),
    "strides_gelu": (128, 132, 128, "gelu", {"strides": True}),
    "strides_gelu_bwd": (128, 132, 128, "gelu_bwd", {"strides": True}),
    "gelu": (256, 192, 128, "gelu", {}),
    "gelu_bwd": (256, 192, 128, "gelu_bwd", {}),
    "head_f32": (256, 180, 192, "f32", {"ldcf": 256, "Mstore": 200}),
    "six_workgroups": (128, 192, 128, "plain", {}),                   # not a multiple of 8: xcd_remap's uneven deal
    "model_dense": (256, 768, 768, "bias_res", {}),
    "model_ffn_gelu": (256, 2048, 768, "gelu", {}),
    "model_ffn_out": (256, 768, 2048, "bias_res", {}),
    "model_ffn_gelu_bwd": (256, 2048, 768, "gelu_bwd", {}),
}


def launch(tile, A, B, N, epi, bias, res, aux, opt):
    """One launch in the form `tile` on sentinel-filled outputs: {name: whole buffer} of C, C2 and Cf."""
    L = _lib.lib()
    pad = 12 if opt.get("strides") else 0
    kw = dict(fill=SENTINEL, Mstore=opt.get("Mstore"), ldc=N + pad, ldc2=N + pad, ldcf=opt.get("ldcf", N + pad))
    try:
        L.plb_set_gemm_nt_tile(tile)
        if epi == "f32":
            # (gemm_nt hands back the output of the launch and C2; C is checked through a buffer of our own)
            Cb = torch.full((A.shape[0], N + pad), SENTINEL, dtype=torch.bfloat16, device=DEV)
            Cf, C2 = gemm_nt(A, B, N, bias=bias, out_f32=True, C=Cb, **kw)
            return {"C": Cb, "C2": C2, "Cf": Cf}
        act = {"plain": 0, "bias_res": 0, "gelu": 1, "gelu_bwd": 2}[epi]
        Cb, C2 = gemm_nt(A, B, N, bias=bias, res=res, aux=aux, act=act, **kw)
        return {"C": Cb, "C2": C2}
    finally:
        L.plb_set_gemm_nt_tile(0)


def untouched(t, rows, cols, what):
    """Everything of buffer t outside [:rows, :cols] still holds the sentinel."""
    s = torch.tensor(SENTINEL, dtype=t.dtype, device=t.device)
    assert bool((t[rows:] == s).all()) and bool((t[:, cols:] == s).all()), f"{what}: written outside {rows} x {cols}"


@pytest.mark.parametrize("name", list(CASES))
def test_64_form_stores_the_bytes_of_the_128_form(name):
    M, N, K, epi, opt = CASES[name]
    seed = 100 + 10 * list(CASES).index(name)
    A = randbf(M, K, seed=seed)
    B = randbf((N + 127) // 128 * 128, K, scale=0.05, seed=seed + 1)     # both forms read whole tiles of B rows: in bounds
    bias = torch.randn(N, generator=torch.Generator().manual_seed(seed + 2)).to(DEV) if epi != "plain" else None
    res = randbf(M, N, seed=seed + 3) if epi == "bias_res" else None
    aux = randbf(M, N, scale=1.5, seed=seed + 4) if epi == "gelu_bwd" else None
    if opt.get("strides"):
        A, B = wide(A, 8), wide(B, 16)
        res = wide(res, 4) if res is not None else None
        aux = wide(aux, 20) if aux is not None else None
    old = launch(-64, A, B, N, epi, bias, res, aux, opt)
    new = launch(64, A, B, N, epi, bias, res, aux, opt)
    for k in old:
        assert torch.equal(bits(old[k]), bits(new[k])), f"{k}: {int((bits(old[k]) != bits(new[k])).sum())} elements differ"

    rows = opt.get("Mstore", M)
    ref = A.double() @ B[:N].double().T
    if bias is not None:
        ref = ref + bias.double()
    if res is not None:
        ref = ref + res.double()
    if aux is not None:
        ref = ref * gelu_grad64(aux)
    ref = ref[:rows]
    for form, out in (("128", old), ("64", new)):
        stored = {"f32": ("Cf",), "gelu": ("C", "C2")}.get(epi, ("C",))
        for k, t in out.items():
            if k in stored:
                untouched(t, rows, N, f"{form} {k}")
            else:
                untouched(t, 0, 0, f"{form} {k} (not an output of this launch)")
        if epi == "f32":
            assert rel_l2(out["Cf"][:rows, :N], ref) < 1e-5, form
            continue
        got = out["C"][:rows, :N].double()
        assert rel_l2(got, ref) < (5e-3 if epi == "gelu_bwd" else 4e-3), form     # bf16 output rounding
        if epi != "gelu_bwd":
            assert float((got - ref).abs().max()) <= 1e-2 * float(ref.abs().max()) + 1e-3, form
        if epi == "gelu":   # C2 = gelu_new of the pre-activation as stored
            assert rel_l2(out["C2"][:rows, :N].double(), gelu64(got)) < 5e-3, form


def _loss_and_grads(eng, args):
    L = _lib.lib()
    out = {}
    try:
        for tile in (-64, 64):
            L.plb_set_gemm_nt_tile(tile)
            loss = eng.loss_fwd_bwd(*args)
            torch.cuda.synchronize()
            out[tile] = (loss.detach().clone(), eng.grads[: eng.trainable].clone())
    finally:
        L.plb_set_gemm_nt_tile(0)
    rows, of = eng.last_application_rows()
    assert rows < of, (rows, of)                      # the last application really ran on the masked rows alone
    (l0, g0), (l1, g1) = out[-64], out[64]
    assert bool(torch.isfinite(l0).all()) and float(g0.abs().max()) > 0.0
    assert torch.equal(bits(l0.float()), bits(l1.float()))
    assert torch.equal(bits(g0), bits(g1)), f"{int((bits(g0) != bits(g1)).sum())} gradient elements differ"


def test_training_call_is_bitwise_the_same_in_both_forms():
    """768/12 at 32 x 512 (the configuration of test_gpu_engine.py's bitwise-repeat test), pruned last application on: the
    compact rows (~2,000) and the phoneme head run on the small kernel; one loss_fwd_bwd per form."""
    pcfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                   max_position_embeddings=512, num_hidden_layers=12)
    labels, masked, lengths, idx = plbert_amd.synthetic_batch(32, 512, seed=4242)
    eng = HipEngine(pcfg, 188, 0, max_batch=32, max_seq=512)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(pcfg, 188, seed=17))
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    _loss_and_grads(eng, (masked, labels, None, off, flat, int(off[-1])))


def test_training_call_is_bitwise_the_same_in_both_forms_ragged_golden():
    """The same on a golden batch with ragged lengths (real_s128_b8: 8 x 128, pruned)."""
    g = load_golden("real_s128_b8")
    ocfg, pcfg, sd = golden_cfg(g)
    B, S = g["labels"].shape
    eng = HipEngine(pcfg, int(g["num_phonemes"]), int(g["num_tokens"]), max_batch=B, max_seq=S)
    eng.load_state_dict(sd)
    idx = [list(map(int, x)) for x in g["index"]]
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    lens = np.asarray([int(x) for x in g["lengths"]], np.int32)
    _loss_and_grads(eng, (g["masked"], g["labels"], lens, off, flat, int(off[-1])))
