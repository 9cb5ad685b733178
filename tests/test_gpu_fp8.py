"""fp8 path (-m gpu; BASELINE.json configs[4]: "fp8 (e4m3) MFMA path for QKV/FFN GEMMs").

The reference has NO fp8 path (it trains under fp16 autocast, configs/config.yml:15), so there is no reference oracle:
parity is against this repository's own bf16 path, as SURVEY.md §7 and BASELINE.md §4 prescribe, and against a CPU
restatement of the fp8 call built on the pinned oracle (oracle/fp8_np.py; last test of this file).
 * kernel level: the fp8 pipeline GEMM against fp32 torch arithmetic on the SAME quantised operands — the only
   difference left is accumulation order, so the tolerance is tight (1e-3 of the output scale after bf16 rounding);
 * step level: loss and gradients of the fp8 step against the bf16 step on identical weights and batch — tolerances
   2e-2 relative on the loss (fp8 carries 3 mantissa bits; the north-star 1e-3 is the bf16-vs-reference bar, not
   this one), per-tensor gradient relative L2 stated at each assertion; then both trainers run 12 steps and must
   descend together.
tests/golden/small_h128 cannot exercise the path (hidden 128 has no pipeline tile; plb_set_fp8 refuses it), so the
reference-captured fixture used is real_s128_b8 (768/12) plus a bench-shaped synthetic batch."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_cfg, load_golden
from gpu_util import assert_fp8_image, rel_l2, site_max, stream
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import HipEngine
from plbert_amd.train import PLBertTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _q(x, scale, bf8):
    dt, mx = (torch.float8_e5m2, 57344.0) if bf8 else (torch.float8_e4m3fn, 448.0)
    q = (x.float() * scale).clamp(-mx, mx).to(dt)
    return q, q.float() / scale


@pytest.mark.parametrize("M,N,K,act,bf8", [(256, 768, 768, 0, 0), (384, 2304, 768, 0, 0), (256, 768, 2048, 0, 1),
                                           (256, 2048, 768, 1, 0), (256, 2048, 768, 2, 1), (128, 1024, 1024, 0, 0)])
def test_fp8_gemm_against_fp32_on_the_same_quantised_operands(M, N, K, act, bf8):
    L = _lib.lib()
    g = torch.Generator(device=DEV).manual_seed(M + N + K + act)
    A = torch.randn(M, K, device=DEV, generator=g) * (0.01 if bf8 else 1.0)
    W = torch.randn(N, K, device=DEV, generator=g) * 0.05
    sa, sw = (57344.0 if bf8 else 448.0) / float(A.abs().max()), 448.0 / float(W.abs().max())
    A8, Ad = _q(A, sa, bf8)
    W8, Wd = _q(W, sw, False)
    bias = torch.randn(N, device=DEV, generator=g) * 0.1
    res = (torch.randn(M, N, device=DEV, generator=g)).to(torch.bfloat16)
    aux = (torch.randn(M, N, device=DEV, generator=g)).to(torch.bfloat16)
    Cb = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    C2 = torch.zeros_like(Cb)
    C8 = torch.full((M, N), 0x55, dtype=torch.uint8, device=DEV)
    deq = torch.tensor([1.0 / sa, 1.0 / sw], device=DEV)
    qs = torch.tensor([3.0], device=DEV)
    amax = torch.zeros(64 * 16, device=DEV)  # one site: 64 slots on separate 64-byte lines
    colp = torch.zeros(2 * (M // 128), N, device=DEV)
    p = _lib.PlbGemmNT()
    p.A, p.lda, p.B, p.ldb = A8.view(torch.uint8).data_ptr(), K, W8.view(torch.uint8).data_ptr(), K
    p.M, p.N, p.K, p.Mstore = M, N, K, M - 3
    p.C, p.ldc, p.C2, p.ldc2 = Cb.data_ptr(), N, C2.data_ptr(), N
    p.deq_a, p.deq_b = deq.data_ptr(), deq.data_ptr() + 4
    if act == 0:
        p.bias, p.res, p.ldr = bias.data_ptr(), res.data_ptr(), N
    if act == 1:
        p.bias = bias.data_ptr()
    if act == 2:
        p.aux, p.ldaux, p.colpart = aux.data_ptr(), N, colp.data_ptr()
    if act:
        p.C8, p.ldc8, p.q_scale, p.q_amax, p.c8_bf8 = C8.data_ptr(), N, qs.data_ptr(), amax.data_ptr(), int(act == 2)
    assert L.plb_launch_gemm_nt_fp8(C.byref(p), act, bf8, stream()) == 0
    torch.cuda.synchronize()
    ref = Ad.double() @ Wd.double().T
    rows = slice(0, M - 3)
    if act == 0:
        want = ref + bias.double() + res.double()
        assert rel_l2(Cb[rows].float(), want[rows].float()) < 4e-3          # bf16 rounding of the output
        assert (Cb[M - 3:] == 0).all()                                       # rows >= Mstore are not stored
    elif act == 1:
        u = (ref + bias.double()).float().to(torch.bfloat16)
        assert rel_l2(Cb[rows].float(), u[rows].float()) < 4e-3
        gl = torch.nn.functional.gelu(Cb.float(), approximate="tanh")
        assert rel_l2(C2[rows].float(), gl[rows]) < 4e-3
        q8 = C8.view(torch.float8_e4m3fn).float() / 3.0                     # the fp8 image of gelu as stored
        assert rel_l2(q8[rows], C2[rows].float()) < 4e-2                     # 3 mantissa bits
        assert abs(float(amax.max()) - float(C2[rows].float().abs().max())) < 1e-6
        assert_fp8_image(C8, C2, qs, 0, rows, amax_site=amax, sentinel=0x55)      # bit for bit, stored rows only
    else:
        x = aux.float()
        k = 0.7978845608028654
        t = torch.tanh(k * (x + 0.044715 * x ** 3))
        dgelu = 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k * (1 + 3 * 0.044715 * x * x)
        want = ref.float() * dgelu
        assert rel_l2(Cb[rows].float(), want[rows]) < 6e-3
        q8 = C8.view(torch.float8_e5m2).float() / 3.0
        assert rel_l2(q8[rows], Cb[rows].float()) < 8e-2                     # 2 mantissa bits
        assert_fp8_image(C8, Cb, qs, 1, rows, amax_site=amax, sentinel=0x55)
        assert rel_l2(colp.sum(0), Cb[rows].float().sum(0)) < 1e-4           # bias-gradient partials of the stored values


def _pair(cfg, B, S, sd=None, seed=0):
    trs = []
    for fp8 in (False, True):
        tr = PLBertTrainer(cfg, 188, max_batch=B, max_seq=S, lr=1e-4, seed=seed, state_dict=sd)
        if fp8:
            tr.engine.set_fp8(True)
        trs.append(tr)
    return trs


def test_fp8_step_against_own_bf16_step_real_model_fixture():
    """real_s128_b8: the reference-captured 768/12 fixture (weights, batch). Call 1 calibrates (bf16 arithmetic: must
    equal the bf16 engine bit for bit), call 2 runs the fp8 GEMMs."""
    g = load_golden("real_s128_b8")
    ocfg, pcfg, sd = golden_cfg(g)
    B, S = g["labels"].shape
    idx = [list(map(int, x)) for x in g["index"]]
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    args = (g["masked"], g["labels"], g["lengths"].astype(np.int32), off, flat, int(off[-1]))
    ref = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S)
    ref.load_state_dict(sd)
    l_ref = float(ref.loss_fwd_bwd(*args).item())
    eng = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S)
    eng.load_state_dict(sd)
    eng.set_fp8(True)
    assert eng.fp8_state() == (True, False)
    l_cal = float(eng.loss_fwd_bwd(*args).item())
    assert l_cal == l_ref and torch.equal(eng.grads, ref.grads)           # calibration call = the bf16 path
    assert eng.fp8_state() == (True, True)
    l_f8 = float(eng.loss_fwd_bwd(*args).item())
    torch.cuda.synchronize()
    assert l_f8 != l_ref                                                     # the fp8 GEMMs really ran
    assert abs(l_f8 - l_ref) / l_ref < 2e-2, (l_f8, l_ref)
    assert abs(l_f8 - float(g["loss"])) / float(g["loss"]) < 2e-2           # and stays near the reference's loss
    lp = "encoder.encoder.albert_layer_groups.0.albert_layers.0."
    for k, tol in ((lp + "ffn.weight", 0.2), (lp + "ffn_output.weight", 0.2), (lp + "attention.query.weight", 0.25),
                   (lp + "attention.dense.weight", 0.2), ("phoneme_predictor.weight", 0.1),
                   ("encoder.embeddings.word_embeddings.weight", 0.25)):
        r = rel_l2(eng.view(k, of=eng.grads), ref.view(k, of=ref.grads))
        assert r < tol, (k, r)
    # validation-only call and switching the mode off again
    l_val = float(eng.loss_fwd(*args).item())
    assert abs(l_val - l_ref) / l_ref < 2e-2
    eng.set_fp8(False)
    assert float(eng.loss_fwd_bwd(*args).item()) == l_ref


def test_fp8_training_descends_with_the_bf16_run():
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  max_position_embeddings=512, num_hidden_layers=4)
    B, S = 8, 512
    labels, masked, lens, idx = plbert_amd.synthetic_batch(B, S, seed=5)
    lens = [512, 512, 400, 512, 300, 512, 512, 77]
    idx = [[i for i in ix if i < n] or [0] for ix, n in zip(idx, lens)]
    for b, n in enumerate(lens):
        labels[b, n:] = 0
        masked[b, n:] = 0
    tb, tf = _pair(cfg, B, S)
    bb, bf = tb.stage_batch(labels, masked, lens, idx), tf.stage_batch(labels, masked, lens, idx)
    lb = [float(tb.step(bb).item()) for _ in range(12)]
    lf = [float(tf.step(bf).item()) for _ in range(12)]
    torch.cuda.synchronize()
    assert lf[0] == lb[0]                                                    # step 1 calibrates in bf16
    assert all(np.isfinite(lf)) and lf[-1] < lf[0] - 0.05                    # it learns
    assert max(abs(a - b) / b for a, b in zip(lf, lb)) < 3e-2, (lf, lb)      # and tracks the bf16 run
    assert not torch.isnan(tf.engine.params).any()


# ---- fp8 forms of the fused epilogues (csrc/gemm_fp8_ln.hip): LayerNorm in the GEMM, gelu-derivative stash -----------
# Operands are quantised with POWER-OF-TWO scales, so the dequantised values are exact in bf16: the bf16 forms of the same
# epilogues (pinned against torch in tests/test_gpu_gemm_ln.py) then compute the very same products, and the only
# difference left is the accumulation order inside the MFMAs.
def _q2(x, bf8, headroom=1.0):
    import math
    mx = 57344.0 if bf8 else 448.0
    scale = 2.0 ** math.floor(math.log2(mx * headroom / float(x.abs().max())))
    q, d = _q(x, scale, bf8)
    return q, d.to(torch.bfloat16), scale


class _F8Ln:
    def __init__(self, M, N, K, bf8, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        A = torch.randn(M, K, device=DEV, generator=g) * (0.02 if bf8 else 1.0)
        W = torch.randn(N, K, device=DEV, generator=g) * K ** -0.5
        self.A8, self.Ad, sa = _q2(A, bf8)
        self.W8, self.Wd, sw = _q2(W, False)
        self.deq = torch.tensor([1.0 / sa, 1.0 / sw], device=DEV)
        self.M, self.N, self.K, self.bf8 = M, N, K, bf8
        self.bias = torch.randn(N, device=DEV, generator=g) * 0.3
        self.res = (torch.randn(M, N, device=DEV, generator=g) * (0.05 if bf8 else 1.0)).to(torch.bfloat16)
        self.gamma = 1.0 + 0.3 * torch.randn(N, device=DEV, generator=g)
        self.beta = 0.2 * torch.randn(N, device=DEV, generator=g)
        nbn = N // (384 if N % 384 == 0 else 256)
        self.xchg = torch.zeros(M // 128 * nbn * nbn * 128 * 2, dtype=torch.int64, device=DEV)
        self.err = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.mean = torch.zeros(M, device=DEV)
        self.rstd = torch.zeros(M, device=DEV)
        self.qs = torch.tensor([4.0 if not bf8 else 2.0 ** 14], device=DEV)
        self.amax = torch.zeros(64 * 16, device=DEV)

    def params(self, fp8):
        p = _lib.PlbGemmNT()
        if fp8:
            p.A, p.B = self.A8.view(torch.uint8).data_ptr(), self.W8.view(torch.uint8).data_ptr()
            p.deq_a, p.deq_b = self.deq.data_ptr(), self.deq.data_ptr() + 4
        else:
            p.A, p.B = self.Ad.data_ptr(), self.Wd.data_ptr()
        p.lda, p.ldb, p.M, p.N, p.K, p.Mstore = self.K, self.K, self.M, self.N, self.K, self.M - 5
        p.ln_gamma, p.ln_beta, p.ln_mean, p.ln_rstd = self.gamma.data_ptr(), self.beta.data_ptr(), self.mean.data_ptr(), self.rstd.data_ptr()
        p.ln_eps, p.ln_xchg, p.ln_err = 1e-12, self.xchg.data_ptr(), self.err.data_ptr()
        return p


@pytest.mark.parametrize("M,N,K", [(1024, 768, 768), (2048, 768, 2048), (1024, 1024, 1024), (1024, 1024, 4096)])
def test_fp8_layernorm_forward_form_against_the_bf16_form(M, N, K):
    L = _lib.lib()
    t = _F8Ln(M, N, K, False, seed=M + N + K)
    outs = []
    for fp8 in (False, True):
        pre = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        y = torch.zeros_like(pre)
        img = torch.full((M, N), 0x55, dtype=torch.uint8, device=DEV)
        p = t.params(fp8)
        p.bias, p.res, p.ldr = t.bias.data_ptr(), t.res.data_ptr(), N
        p.C, p.ldc, p.C2, p.ldc2 = pre.data_ptr(), N, y.data_ptr(), N
        if fp8:
            p.C8, p.ldc8, p.q_scale, p.q_amax, p.c8_bf8 = img.data_ptr(), N, t.qs.data_ptr(), t.amax.data_ptr(), 0
            assert L.plb_launch_gemm_nt_fp8_ln(C.byref(p), 5, 0, stream()) == 0
        else:
            assert L.plb_launch_gemm_nt_ln(C.byref(p), 5, stream()) == 0
        torch.cuda.synchronize()
        outs.append((pre, y, t.mean.clone(), t.rstd.clone(), img))
    (pre0, y0, m0, r0, _), (pre1, y1, m1, r1, img) = outs
    rows = slice(0, M - 5)
    assert rel_l2(pre1[rows].float(), pre0[rows].float()) < 2e-3           # same products, other accumulation order, bf16 store
    assert rel_l2(y1[rows].float(), y0[rows].float()) < 3e-3
    assert (m1[rows] - m0[rows]).abs().max() < 2e-3 and ((r1[rows] - r0[rows]) / r0[rows]).abs().max() < 2e-3
    q = img.view(torch.float8_e4m3fn).float() / 4.0
    assert rel_l2(q[rows], y1[rows].float()) < 4e-2                          # the image is the stored bf16 row, 3 mantissa bits
    assert (q[rows] - y1[rows].float()).abs().max() <= 2.0 ** -4 * float(y1[rows].float().abs().max()) + 1e-6
    assert (img[M - 5:] == 0x55).all() and (y1[M - 5:] == 0).all()           # rows >= Mstore: untouched
    assert abs(float(t.amax.max()) - float(y1[rows].float().abs().max())) < 1e-6
    assert_fp8_image(img, y1, t.qs, 0, rows, amax_site=t.amax, sentinel=0x55)
    assert int(t.err[0].item()) == 0 and int(t.xchg.abs().sum().item()) == 0


@pytest.mark.parametrize("M,N,K", [(1024, 768, 2048), (2048, 768, 2304), (1024, 1024, 4096), (1024, 1024, 3072)])
def test_fp8_layernorm_backward_form_against_the_bf16_form(M, N, K):
    """Operand A is a gradient: e5m2 image."""
    L = _lib.lib()
    t = _F8Ln(M, N, K, True, seed=M + N + K + 1)
    pre = (torch.randn(M, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))).to(torch.bfloat16)
    x = pre.float()
    t.mean.copy_(x.mean(1)); t.rstd.copy_((x.var(1, unbiased=False) + 1e-12).rsqrt())
    outs = []
    for fp8 in (False, True):
        dx = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        colp = torch.full((2 * M // 128, 3, N), 9.0, device=DEV)
        img = torch.full((M, N), 0x55, dtype=torch.uint8, device=DEV)
        p = t.params(fp8)
        p.res, p.ldr, p.aux, p.ldaux = t.res.data_ptr(), N, pre.data_ptr(), N
        p.C, p.ldc, p.colpart = dx.data_ptr(), N, colp.data_ptr()
        if fp8:
            p.C8, p.ldc8, p.q_scale, p.q_amax, p.c8_bf8 = img.data_ptr(), N, t.qs.data_ptr(), t.amax.data_ptr(), 1
            assert L.plb_launch_gemm_nt_fp8_ln(C.byref(p), 6, 1, stream()) == 0
        else:
            assert L.plb_launch_gemm_nt_ln(C.byref(p), 6, stream()) == 0
        torch.cuda.synchronize()
        outs.append((dx, colp, img))
    (dx0, c0, _), (dx1, c1, img) = outs
    rows = slice(0, M - 5)
    assert rel_l2(dx1[rows].float(), dx0[rows].float()) < 4e-3
    for k in range(3):
        assert rel_l2(c1.double().sum(0)[k], c0.double().sum(0)[k]) < 2e-3
    q = img.view(torch.float8_e5m2).float() / float(t.qs.item())
    assert rel_l2(q[rows], dx1[rows].float()) < 8e-2                         # 2 mantissa bits
    assert (img[M - 5:] == 0x55).all()
    assert abs(float(t.amax.max()) - float(dx1[rows].float().abs().max())) < 1e-6
    assert_fp8_image(img, dx1, t.qs, 1, rows, amax_site=t.amax, sentinel=0x55)
    assert int(t.err[0].item()) == 0 and int(t.xchg.abs().sum().item()) == 0


@pytest.mark.parametrize("M,N,K,with16", [(256, 2048, 768, True), (1024, 2048, 768, False), (384, 4096, 1024, True)])
def test_fp8_gelu_stash_forms_forward_then_backward(M, N, K, with16):
    """FFN up-projection + gelu_new with the derivative stashed, and the matching backward, on fp8 operands. The stash is
    private to the pair of launches (lane layout of the 128x256 tile): it is checked through the backward's result.
    with16 = False: gelu(u) and dU leave as their 1-byte images alone (what an fp8 training call does)."""
    L = _lib.lib()
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    A8, Ad, sa = _q2(torch.randn(M, K, device=DEV, generator=g), False)
    W8, Wd, sw = _q2(torch.randn(N, K, device=DEV, generator=g) * K ** -0.5, False)
    bias = torch.randn(N, device=DEV, generator=g) * 0.3
    deq = torch.tensor([1.0 / sa, 1.0 / sw], device=DEV)
    stash = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
    gl = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
    g8buf = torch.full((M + 2, N), 0x55, dtype=torch.uint8, device=DEV)   # two rows past the output: must stay untouched
    g8 = g8buf[:M]
    qs = torch.tensor([16.0], device=DEV)
    amax = torch.zeros(64 * 16, device=DEV)
    p = _lib.PlbGemmNT()
    p.A, p.lda, p.B, p.ldb = A8.view(torch.uint8).data_ptr(), K, W8.view(torch.uint8).data_ptr(), K
    p.M, p.N, p.K, p.Mstore = M, N, K, M
    p.deq_a, p.deq_b, p.bias = deq.data_ptr(), deq.data_ptr() + 4, bias.data_ptr()
    p.C, p.ldc = stash.data_ptr(), N
    if with16:
        p.C2, p.ldc2 = gl.data_ptr(), N
    p.C8, p.ldc8, p.q_scale, p.q_amax, p.c8_bf8 = g8.data_ptr(), N, qs.data_ptr(), amax.data_ptr(), 0
    assert L.plb_launch_gemm_nt_fp8_gelud(C.byref(p), 0, 0, stream()) == 0
    torch.cuda.synchronize()
    u = (Ad.double() @ Wd.double().T + bias.double()).float().requires_grad_(True)
    ref_g = torch.nn.functional.gelu(u, approximate="tanh")
    q = g8.view(torch.float8_e4m3fn).float() / 16.0
    assert rel_l2(q, ref_g.detach()) < 4e-2
    if with16:
        assert rel_l2(gl.float(), ref_g.detach()) < 4e-3
        assert rel_l2(q, gl.float()) < 4e-2
        assert abs(float(amax.max()) - float(gl.float().abs().max())) < 1e-6
        assert_fp8_image(g8buf, gl, qs, 0, slice(0, M), amax_site=amax, sentinel=0x55)
    else:
        assert (gl == 7.0).all()                                             # no bf16 image was written
        # the image-only launch writes the same bytes as a launch that also stores gelu(u) — the image of those values
        g8b = torch.full((M + 2, N), 0x55, dtype=torch.uint8, device=DEV)
        amax_b = torch.zeros(64 * 16, device=DEV)
        p.C2, p.ldc2, p.C8, p.q_amax = gl.data_ptr(), N, g8b.data_ptr(), amax_b.data_ptr()
        assert L.plb_launch_gemm_nt_fp8_gelud(C.byref(p), 0, 0, stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(g8b[:M], g8) and site_max(amax_b) == site_max(amax)
        assert_fp8_image(g8b, gl, qs, 0, slice(0, M), amax_site=amax_b, sentinel=0x55)
    # backward: dU = (dY·W2ᵀ) ∘ gelu'(u) with a gradient operand in e5m2
    K2 = 768 if K == 768 else 1024
    D8, Dd, sd = _q2(torch.randn(M, K2, device=DEV, generator=g) * 0.01, True)
    V8, Vd, sv = _q2(torch.randn(N, K2, device=DEV, generator=g) * K2 ** -0.5, False)
    deq2 = torch.tensor([1.0 / sd, 1.0 / sv], device=DEV)
    du = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
    du8buf = torch.full((M + 2, N), 0x55, dtype=torch.uint8, device=DEV)
    du8 = du8buf[:M]
    colp = torch.zeros(2 * (M // 128), N, device=DEV)
    qs2 = torch.tensor([2.0 ** 16], device=DEV)
    amax2 = torch.zeros(64 * 16, device=DEV)
    p2 = _lib.PlbGemmNT()
    p2.A, p2.lda, p2.B, p2.ldb = D8.view(torch.uint8).data_ptr(), K2, V8.view(torch.uint8).data_ptr(), K2
    p2.M, p2.N, p2.K, p2.Mstore = M, N, K2, M
    p2.deq_a, p2.deq_b = deq2.data_ptr(), deq2.data_ptr() + 4
    p2.aux, p2.ldaux, p2.colpart = stash.data_ptr(), N, colp.data_ptr()
    if with16:
        p2.C, p2.ldc = du.data_ptr(), N
    p2.C8, p2.ldc8, p2.q_scale, p2.q_amax, p2.c8_bf8 = du8.data_ptr(), N, qs2.data_ptr(), amax2.data_ptr(), 1
    assert L.plb_launch_gemm_nt_fp8_gelud(C.byref(p2), 1, 1, stream()) == 0
    torch.cuda.synchronize()
    dg = (Dd.double() @ Vd.double().T).float()
    ref_g.backward(dg)
    want = u.grad
    got8 = du8.view(torch.float8_e5m2).float() / 2.0 ** 16
    assert rel_l2(got8, want) < 8e-2
    if with16:
        assert rel_l2(du.float(), want) < 8e-3                              # the derivative went through one bf16 rounding
        assert rel_l2(colp.sum(0), du.float().sum(0)) < 1e-4
        assert abs(float(amax2.max()) - float(du.float().abs().max())) < 1e-9
        assert_fp8_image(du8buf, du, qs2, 1, slice(0, M), amax_site=amax2, sentinel=0x55)
    else:
        assert (du == 7.0).all()
        assert rel_l2(colp.sum(0), want.sum(0)) < 2e-2
        du8b = torch.full((M + 2, N), 0x55, dtype=torch.uint8, device=DEV)
        amax_b2 = torch.zeros(64 * 16, device=DEV)
        p2.C, p2.ldc, p2.C8, p2.q_amax = du.data_ptr(), N, du8b.data_ptr(), amax_b2.data_ptr()
        assert L.plb_launch_gemm_nt_fp8_gelud(C.byref(p2), 1, 1, stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(du8b[:M], du8) and site_max(amax_b2) == site_max(amax2)
        assert_fp8_image(du8b, du, qs2, 1, slice(0, M), amax_site=amax_b2, sentinel=0x55)


@pytest.mark.parametrize("Mtot,N,K,splits", [(8192, 768, 768, 28), (8192, 2304, 768, 9), (12288, 768, 2048, 10),
                                            (8192, 256, 256, 1), (16384, 2048, 768, 10), (8192 + 128, 1024, 1024, 16)])
def test_fp8_weight_gradient_gemm(Mtot, N, K, splits):
    """dW[N,K] = A^T·B over token rows on 1-byte token-major images (csrc/gemm_tn_fp8.hip: ds_read_b64_tr_b8 fragments,
    block-scaled fp8 MFMA): e5m2 gradient image x e4m3 activation image, against fp64 on the dequantised operands — the
    only difference is the accumulation order (fp32 inside the kernel, fixed-order slab reduction)."""
    L = _lib.lib()
    g = torch.Generator(device=DEV).manual_seed(Mtot + N + K)
    A8, Ad, sa = _q2(torch.randn(Mtot, N, device=DEV, generator=g) * 0.01, True)
    B8, Bd, sb = _q2(torch.randn(Mtot, K, device=DEV, generator=g), False)
    deq = torch.tensor([1.0 / sa, 1.0 / sb], device=DEV)
    rps = -(-Mtot // splits)
    rps = (rps + 127) // 128 * 128
    splits = -(-Mtot // rps)
    slab = torch.zeros(splits, N, K, device=DEV)
    out = torch.zeros(N, K, device=DEV)
    p = _lib.PlbGemmTN()
    p.A, p.lda, p.Ncols, p.B, p.ldb = A8.view(torch.uint8).data_ptr(), N, N, B8.view(torch.uint8).data_ptr(), K
    p.Mtot, p.N, p.K, p.rows_per_split, p.splits, p.slab = Mtot, N, K, rps, splits, slab.data_ptr()
    p.deq_a, p.deq_b = deq.data_ptr(), deq.data_ptr() + 4
    assert L.plb_launch_gemm_tn_fp8(C.byref(p), stream()) == 0
    assert L.plb_launch_reduce_slabs(slab.data_ptr(), splits, N * K, out.data_ptr(), 0, stream()) == 0
    torch.cuda.synchronize()
    want = (Ad.double().T @ Bd.double()).float()
    assert rel_l2(out, want) < 5e-5                                          # fp32 accumulation over >= 8192 rows
    # and bitwise reproducible
    out2 = torch.zeros_like(out)
    assert L.plb_launch_gemm_tn_fp8(C.byref(p), stream()) == 0
    assert L.plb_launch_reduce_slabs(slab.data_ptr(), splits, N * K, out2.data_ptr(), 0, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, out2)


def test_fp8_forward_on_an_inference_engine():
    """plb_forward / plb_loss_fwd in fp8 mode on an engine built without training buffers (one layer of activations, one
    set of 1-byte images, no transposed weight copies): the calibration call equals the bf16 engine bit for bit, the fp8
    calls stay close to it and agree with each other."""
    g = load_golden("real_s128_b8")
    ocfg, pcfg, sd = golden_cfg(g)
    B, S = g["labels"].shape
    lens = g["lengths"].astype(np.int32)
    ref = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S, train=False)
    ref.load_state_dict(sd)
    _, ph_ref, _ = ref.forward(g["masked"], lens)
    eng = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S, train=False)
    eng.load_state_dict(sd)
    eng.set_fp8(True)
    _, ph_cal, _ = eng.forward(g["masked"], lens)
    assert torch.equal(ph_cal, ph_ref)
    _, ph8, _ = eng.forward(g["masked"], lens)
    _, ph8b, _ = eng.forward(g["masked"], lens)
    torch.cuda.synchronize()
    v = torch.from_numpy(np.arange(S)[None, :] < lens[:, None]).to(ph8.device)
    assert not torch.equal(ph8, ph_ref)                                       # the fp8 GEMMs really ran
    r, a, rr = rel_l2(ph8[v], ph_ref[v]), float((ph8[v] - ph_ref[v]).abs().max()), rel_l2(ph8b[v], ph8[v])
    print(f"fp8 inference logits vs bf16: rel L2 {r:.4f}, max abs {a:.4f}; consecutive fp8 calls rel L2 {rr:.4f}")
    assert r < 0.1 and a < 0.5, (r, a)
    assert rr < 5e-2, rr                                                      # delayed scales moved a little between the calls
    assert bool(torch.isfinite(ph8[v]).all())
    off, flat = plbert_amd.masked_indices_to_csr([list(map(int, x)) for x in g["index"]])
    l8 = float(eng.loss_fwd(g["masked"], g["labels"], lens, off, flat, int(off[-1])).item())
    assert abs(l8 - float(g["loss"])) / float(g["loss"]) < 2e-2


@pytest.mark.parametrize("B,S,lens", [(3, 512, [512, 512, 512]), (5, 200, [200, 180, 77, 200, 13])])
def test_fp8_step_on_shapes_without_fused_layernorm_forms(B, S, lens):
    """Token counts that are no multiple of 1024 take the unfused path (GEMM + LayerNorm kernel, which then writes the
    1-byte images), ragged rows included; 3 x 512: weight gradients on the images (12 x 1536 rows), 5 x 200 (1024 padded
    rows -> fused again, but ragged and below the weight-gradient GEMM's row minimum on a 4-layer model): bf16 operands."""
    layers = 12 if B == 3 else 4
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  max_position_embeddings=512, num_hidden_layers=layers)
    labels, masked, _, idx = plbert_amd.synthetic_batch(B, S, seed=17)
    idx = [[i for i in ix if i < n] or [0] for ix, n in zip(idx, lens)]
    for b, n in enumerate(lens):
        labels[b, n:] = 0
        masked[b, n:] = 0
    sd = plbert_amd.deterministic_state_dict(cfg, 188, seed=9)
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    args = (masked, labels, np.asarray(lens, np.int32), off, flat, int(off[-1]))
    ref = HipEngine(cfg, 188, 0, max_batch=B, max_seq=S)
    ref.load_state_dict(sd)
    l_ref = float(ref.loss_fwd_bwd(*args).item())
    eng = HipEngine(cfg, 188, 0, max_batch=B, max_seq=S)
    eng.load_state_dict(sd)
    eng.set_fp8(True)
    assert float(eng.loss_fwd_bwd(*args).item()) == l_ref and torch.equal(eng.grads, ref.grads)   # calibration call
    l8 = float(eng.loss_fwd_bwd(*args).item())
    l8b = float(eng.loss_fwd_bwd(*args).item())
    torch.cuda.synchronize()
    n = eng.trainable
    r = rel_l2(eng.grads[:n], ref.grads[:n])
    assert l8 != l_ref and abs(l8 - l_ref) / l_ref < 2e-2 and abs(l8b - l_ref) / l_ref < 2e-2, (l8, l8b, l_ref)
    assert r < 0.2, r
    assert bool(torch.isfinite(eng.grads[:n]).all())
    assert eng.status()["ln_exchange_timeouts"] == 0


def test_fp8_weight_gradients_with_padded_token_rows_after_a_larger_call():
    """The fp8 weight-gradient GEMMs sum over ALL Tp = ceil128(T) rows of every application, pad rows included, so they
    rely on: every e5m2 gradient image has zero pad rows (dq8 memset, ln_bwd_wide zeroes its out8, the fused forms compute
    zeros), and the pad rows of the e4m3 activation images hold FINITE bytes (x8 / a8 / g8 are rewritten over all Tp rows;
    c8, the attention context image, only over the T valid rows — its pad rows keep what an earlier, LARGER call left
    there). 7 x 500 = 3,500 tokens -> Tp = 3,584, 12 x 3,584 = 43,008 stacked rows: the images path (tn8), ragged rows,
    84 pad rows per application that the 8 x 512 calls before it filled with real activations. Stale bytes times zero
    gradients must add nothing: gradients as close to the bf16 path as on a fresh engine."""
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  max_position_embeddings=512, num_hidden_layers=12)
    sd = plbert_amd.deterministic_state_dict(cfg, 188, seed=9)

    def batch(B, S, lens, seed):
        labels, masked, _, idx = plbert_amd.synthetic_batch(B, S, seed=seed)
        idx = [[i for i in ix if i < n] or [0] for ix, n in zip(idx, lens)]
        for b, n in enumerate(lens):
            labels[b, n:] = 0
            masked[b, n:] = 0
        off, flat = plbert_amd.masked_indices_to_csr(idx)
        return (masked, labels, np.asarray(lens, np.int32), off, flat, int(off[-1]))

    big = batch(8, 512, [512] * 8, seed=3)
    small = batch(7, 500, [500, 500, 480, 500, 333, 500, 91], seed=4)
    ref = HipEngine(cfg, 188, 0, max_batch=8, max_seq=512)
    ref.load_state_dict(sd)
    l_ref = float(ref.loss_fwd_bwd(*small).item())
    n = ref.trainable
    g_ref = ref.grads[:n].clone()
    res = {}
    for stale in (False, True):
        eng = HipEngine(cfg, 188, 0, max_batch=8, max_seq=512)
        eng.load_state_dict(sd)
        eng.set_fp8(True)
        if stale:   # fills every image's rows [0, 4096) of every application, pad rows of the small call included
            eng.loss_fwd_bwd(*big)
            eng.loss_fwd_bwd(*big)
        eng.loss_fwd_bwd(*small)                      # (fresh engine: the calibration call)
        l8 = float(eng.loss_fwd_bwd(*small).item())
        l8 = float(eng.loss_fwd_bwd(*small).item())   # scales learnt on this very batch in both engines
        torch.cuda.synchronize()
        assert bool(torch.isfinite(eng.grads[:n]).all())
        res[stale] = (l8, rel_l2(eng.grads[:n], g_ref), eng.grads[:n].clone())
        assert eng.status()["ln_exchange_timeouts"] == 0
        del eng
    for stale in (False, True):
        l8, r, _ = res[stale]
        assert abs(l8 - l_ref) / l_ref < 2e-2, (stale, l8, l_ref)
        assert r < 0.15, (stale, r)                   # whole-gradient distance of the fp8 path: 0.10-0.11 everywhere
    # the same call on the same weights with the same scales' history on this batch: only rounding chaos may differ
    assert abs(res[True][1] - res[False][1]) < 0.02, (res[True][1], res[False][1])


def test_fp8_clamped_calls_are_counted_and_the_gradient_history_holds_the_scale():
    """Delayed scaling has a blind spot: a call whose gradients are several times the previous call's is quantised under the
    old scale and the excess is clamped (include/plbert.h: plb_fp8_stats). One sample after sixteen: the loss is a mean
    over samples, so every gradient is ~16x larger -> beyond the 2x headroom of the e5m2 sites: that call must be COUNTED
    (clamped_calls, worst overshoot > 1), the next call on the same batch must not be (the scale has followed), and going
    back to the large batch must not clamp either — the four-call history keeps the larger maximum."""
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  max_position_embeddings=512, num_hidden_layers=2)
    sd = plbert_amd.deterministic_state_dict(cfg, 188, seed=9)
    eng = HipEngine(cfg, 188, 0, max_batch=16, max_seq=512)
    eng.load_state_dict(sd)
    eng.set_fp8(True)

    def call(B):
        labels, masked, lens, idx = plbert_amd.synthetic_batch(B, 512, seed=21)
        off, flat = plbert_amd.masked_indices_to_csr(idx)
        return float(eng.loss_fwd_bwd(masked, labels, None, off, flat, int(off[-1])).item())

    grad_sites = ("dpre2", "dU", "dpre1", "dQKV")
    call(16); call(16); call(16)
    st = eng.fp8_stats()
    assert all(st[k] == (0, 0.0) for k in st), st                       # steady batches: nothing clamped anywhere
    call(2)                                                              # 8x the gradients under the 16-sample scales
    st = eng.fp8_stats()
    assert all(st[k][0] == 1 and st[k][1] > 1.5 for k in grad_sites), st
    call(2)
    assert all(eng.fp8_stats()[k][0] == 1 for k in grad_sites)          # the scale has followed
    l_back = call(16)
    st = eng.fp8_stats()
    assert all(st[k][0] == 1 for k in grad_sites), st                   # back to small gradients: coarser, never clamped
    assert np.isfinite(l_back)


def _fp8_vs_bf16(cfg, B, S, num_tokens=0, seed=5):
    labels, masked, lens, idx = plbert_amd.synthetic_batch(B, S, seed=seed)
    sd = plbert_amd.deterministic_state_dict(cfg, 188, num_tokens, seed=seed)
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    tok = np.random.RandomState(seed).randint(0, num_tokens, size=(B, S)).astype(np.int64) if num_tokens else None
    out = []
    for fp8 in (False, True):
        eng = HipEngine(cfg, 188, num_tokens, max_batch=B, max_seq=S)
        eng.load_state_dict(sd)
        if fp8:
            eng.set_fp8(True)
            eng.loss_fwd_bwd(masked, labels, None, off, flat, int(off[-1]), token_ids=tok)   # calibration
        loss = float(eng.loss_fwd_bwd(masked, labels, None, off, flat, int(off[-1]), token_ids=tok).item())
        torch.cuda.synchronize()
        n = eng.total if num_tokens else eng.trainable
        g = torch.cat([eng.grads[: eng.trainable], eng.grads[eng.token_range[0]:eng.token_range[1]]]) if num_tokens else eng.grads[:n]
        out.append((loss, g.clone()))
        del eng
    return out


def test_fp8_dual_head_step():
    """MultiTaskModel step (phoneme + token loss) in fp8 mode: the encoder's GEMMs run on the images, the token head's
    fused GEMM + cross-entropy passes stay bf16 and add their gradient into dH before the layer loop."""
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  max_position_embeddings=512, num_hidden_layers=4)
    (l0, g0), (l1, g1) = _fp8_vs_bf16(cfg, 4, 512, num_tokens=1024)
    assert l1 != l0 and abs(l1 - l0) / l0 < 2e-2, (l0, l1)
    assert rel_l2(g1, g0) < 0.2 and bool(torch.isfinite(g1).all())


def test_fp8_with_bf16_weight_gradient_operands(monkeypatch):
    """PLBERT_FP8_TN=0: the fp8 step with the weight-gradient GEMMs on the bf16 stash (gelu(u), dU, dQKV then leave in both
    forms) — the fall-back the engine also takes below the fp8 kernel's row minimum."""
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  max_position_embeddings=512, num_hidden_layers=12)
    (l0, g0), (l1, g1) = _fp8_vs_bf16(cfg, 2, 512)
    monkeypatch.setenv("PLBERT_FP8_TN", "0")
    (_, _), (l2, g2) = _fp8_vs_bf16(cfg, 2, 512)
    assert abs(l1 - l0) / l0 < 2e-2 and abs(l2 - l0) / l0 < 2e-2
    assert rel_l2(g1, g0) < 0.2 and rel_l2(g2, g0) < 0.2
    assert l1 == l2 and not torch.equal(g1, g2)        # same forward; the weight gradients come from other operands
    assert rel_l2(g2, g1) < 0.1


@pytest.mark.parametrize("L,B,lens,tn8", [(1, 16, None, True), (4, 4, None, True), (4, 4, [512, 401, 77, 512], False)])
def test_fp8_step_against_the_fp8_restatement(L, B, lens, tn8, monkeypatch):
    """The fp8 call against oracle/fp8_np.py — the oracle's arithmetic with the operands of the layer's GEMMs rounded to
    e4m3 / e5m2 at the same sites under the same delayed scales, and bfloat16 wherever the device stores bfloat16.
    The fp8 step sits ~0.06-0.1 (relative L2, per tensor) from the un-rounded oracle: that is the 3-bit mantissa. From the
    restatement it must sit closer, tensor by tensor — what is left are rounding-boundary flips: a value the two
    computations see 1e-4 apart lands on different sides of an fp8 boundary with probability (difference / fp8 ulp), a
    flip is a full ulp, and its effect seeds flips at the next site, so the distance grows along the chain of sites instead
    of vanishing (measured, profiles/r04_fp8_restatement.txt): one application: 3-8x closer for the tensors the backward
    reaches first (head, LayerNorm 2, ffn_output, ffn.bias), 2-3x for the attention weights at the end of the chain;
    four applications: 1.6-2.4x throughout. A wrong scale, format, site or dequantisation factor would put the step no
    closer to the restatement than to the oracle. The bf16 (calibration) call is held to its bf16 restatement likewise.
    768-wide; 16 x 512 tokens x 1 application and 4 x 512 x 4: 8192 stacked rows, the smallest case the fp8 weight-
    gradient GEMM takes (tn8); the ragged case runs with PLBERT_FP8_TN=0 (weight gradients from the bf16 tensors)."""
    from oracle import fp8_np
    from oracle.albert_np import Config
    if not tn8:
        monkeypatch.setenv("PLBERT_FP8_TN", "0")
    S = 512
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  max_position_embeddings=512, num_hidden_layers=L)
    ocfg = Config(hidden_size=768, num_attention_heads=12, intermediate_size=2048, num_hidden_layers=L)
    sd = plbert_amd.deterministic_state_dict(cfg, 188, seed=5)
    labels, masked, full, idx = plbert_amd.synthetic_batch(B, S, seed=5)
    lens = [int(x) for x in (full if lens is None else lens)]
    idx = [[i for i in ix if i < n] or [0] for ix, n in zip(idx, lens)]
    for b, n in enumerate(lens):
        labels[b, n:] = 0
        masked[b, n:] = 0
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    args = (masked, labels, np.asarray(lens, np.int32), off, flat, int(off[-1]))
    eng = HipEngine(cfg, 188, 0, max_batch=B, max_seq=S)
    eng.load_state_dict(sd)
    eng.set_fp8(True)
    l_cal = float(eng.loss_fwd_bwd(*args).item())                 # calibration: bf16 arithmetic, records the maxima
    g_cal = eng.grads.clone()
    l8 = float(eng.loss_fwd_bwd(*args).item())                    # fp8 call under the scales those maxima give
    torch.cuda.synchronize()
    o_l0, _, G0, _ = fp8_np.loss_and_grads_fp8(ocfg, sd, masked, labels, lens, idx)                      # == oracle/albert_np.py
    o_l16, _, G16, amax = fp8_np.loss_and_grads_fp8(ocfg, sd, masked, labels, lens, idx, bf16=True, dtype=np.float32,
                                                    prune_last=L >= 2)
    # (the device evaluates the last application's post-attention part on the masked rows only, in bf16: restated too)
    pruned = eng.last_application_rows()
    assert (pruned[0] < pruned[1]) == (L >= 2)
    o_l8, _, G8, _ = fp8_np.loss_and_grads_fp8(ocfg, sd, masked, labels, lens, idx, amax=amax, tn8=tn8, bf16=True,
                                               dtype=np.float32, prune_last=pruned[0] < pruned[1])
    assert abs(l_cal - o_l0) / o_l0 < 1e-3, (l_cal, o_l0)           # the bf16 call against the oracle (north-star bar)
    print(f"\nloss: hip fp8 {l8:.6f}, restated fp8 {o_l8:.6f}; hip bf16 {l_cal:.6f}, restated bf16 {o_l16:.6f}, oracle {o_l0:.6f}")
    lp = "encoder.encoder.albert_layer_groups.0.albert_layers.0."
    big = [lp + "attention.query.weight", lp + "attention.key.weight", lp + "attention.value.weight", lp + "attention.dense.weight",
           lp + "ffn.weight", lp + "ffn_output.weight"]
    rest = [lp + "ffn.bias", lp + "attention.LayerNorm.weight", lp + "full_layer_layer_norm.weight",
            "encoder.encoder.embedding_hidden_mapping_in.weight", "encoder.embeddings.word_embeddings.weight",
            "phoneme_predictor.weight"]
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    rows = []
    for k in big + rest:
        got = eng.view(k, of=eng.grads).double().cpu().numpy()
        cal = eng.view(k, of=g_cal).double().cpu().numpy()
        rows.append((k, rel(got, G8[k]), rel(got, G0[k]), rel(cal, G16[k]), rel(cal, G0[k])))
        print(f"{k[-40:]:>40s}: fp8 vs restated fp8 {rows[-1][1]:.4f}, vs oracle {rows[-1][2]:.4f};   "
              f"bf16 vs restated bf16 {rows[-1][3]:.4f}, vs oracle {rows[-1][4]:.4f}")
    assert abs(l8 - o_l8) / o_l8 < 5e-4, (l8, o_l8, o_l0)
    early = {lp + "ffn_output.weight", lp + "ffn.bias", lp + "full_layer_layer_norm.weight", "phoneme_predictor.weight"}
    for k, r_emul, r_plain, r16_emul, r16_plain in rows:
        assert r_emul < 0.06, (k, r_emul, r_plain)
        # (four applications: 0.52-0.72 measured on the shipped build, the word embeddings — the end of the chain — closest to the bound)
        assert r_emul < (0.8 if L > 1 else 0.35 if k in early else 0.6) * r_plain, (k, r_emul, r_plain)
        assert r16_emul < 0.8 * r16_plain and r16_plain < 0.02, (k, r16_emul, r16_plain)
