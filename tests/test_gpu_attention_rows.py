"""-m gpu: attention parity PER ROW against float64, with the tolerance taken from a rounding model.

The aggregate tests (test_gpu_kernels.py: rel_l2 < 6e-3 for ctx, < 1.5e-2 for dq / dk / dv) cannot see a fault confined to
a few rows. Here every (token row, head) of ctx, dq, dk and dv is held to gpu_util.attention_fp64 within 4 x the WORST row
of gpu_util.attention_rounded (float64 with the bf16 / fp32 roundings the kernels make) on the same inputs; lse per element
(2e-3), delta of the two-kernel form per row (1e-5 of sum |dO.O|), padded rows exactly zero, and the number of rows that
fall under the absolute check (zero reference) equal to the number the lengths predict. gpu_util.check_rows is the checker;
tests/test_attention_rows_host.py shows on the CPU that it catches a one-row defect the aggregates miss.

Cases: every edge of the 32-query wave, the 64-key tile and the 128-row query tile as a length; sequences that end inside
a tile; a sharp (near one-hot) and a flat softmax; heads of different magnitude; compact queries.

Maxima of the row error of the model (attention_rounded against attention_fp64; the bound is 4 x these) and of the kernels
on an MI355X, from the lines a -s run prints per case and form (`rows <case> form <f>: <output> model <max> kernel <max>`).
The two forms of the backward are different kernels that agree bit for bit on all but a few elements (edges: 407 of
1,474,560 elements of dqkv differ, sharp: 109 of 196,608), and the maxima they print coincide in every case to the digits
shown: one kernel column serves both forms.

              model                                        kernel (form 0 and form 1)
    case      ctx        dq         dk         dv          ctx        dq         dk         dv
    edges     3.32e-03   4.13e-03   4.02e-03   3.84e-03    3.78e-03   4.09e-03   4.01e-03   3.85e-03
    tail130   3.43e-03   4.43e-03   4.91e-03   4.22e-03    3.43e-03   4.43e-03   4.91e-03   4.22e-03
    tail40    2.91e-03   2.84e-02   9.79e-03   3.20e-03    2.91e-03   2.84e-02   9.79e-03   3.20e-03
    tail600   3.46e-03   4.11e-03   3.77e-03   3.53e-03    3.48e-03   4.11e-03   3.79e-03   3.53e-03   (form 0 only)
    sharp     2.99e-03   6.39e+00   8.42e-01   4.36e-03    4.16e-03   6.39e+00   1.02e+00   4.36e-03
    flat      2.75e-03   3.31e-03   3.30e-03   3.14e-03    2.69e-03   3.31e-03   3.29e-03   3.14e-03
    heads     3.05e-03   3.81e-02   1.03e-02   3.84e-03    3.64e-03   3.81e-02   1.03e-02   3.84e-03
    compact   3.07e-03   3.59e-03   4.03e-03   3.65e-03    3.26e-03   3.70e-03   4.05e-03   3.65e-03   (form 0 only)

sharp: a row whose P is 0.9999 on one key has dS = P (dP - delta) a thousand times smaller than the bf16 rounding of the
context that delta is formed from, so dq / dk of such rows are ill-conditioned for ANY kernel that reads a bf16 context: the
model's worst row is off by several times its own norm, and the bound follows it. ctx and dv stay at 3e-3 to 4e-3.
"""
import ctypes as C

import pytest
import torch

from plbert_amd import _lib
from gpu_util import (ATTN_SCALE, attention_delta_terms, attention_fp64, attention_rounded, attn_args, bwd_form,  # noqa: F401
                      check_delta, check_rows, stream)

pytestmark = pytest.mark.gpu
DEV = "cuda"

EDGES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256]


def randn(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g)


def plain_inputs(B, S, NH, lens, seed, qscale=1.0, head_scales=None):
    x = randn(B * S, 3, NH, 64, seed=seed)
    x[:, 0] *= qscale
    if head_scales:   # head h: V x a_h, Q and K x sqrt(a_h) — outputs differ in size by head, the scores' spread is a_h
        a = torch.tensor(head_scales).reshape(1, 1, NH, 1)
        x *= torch.cat([a.sqrt(), a.sqrt(), a], dim=1)
    return x.reshape(B * S, 3 * NH * 64)


def sharp_inputs(B, S, NH, lens, seed):
    """Q = 4 u; key (r * 37) mod len of query r is u_r plus noise of 0.3, so its scaled score is 4 |u|^2 / 8 = 32 +- 1.2.
    With independent u the other keys would score 0 +- 4 and P would be one-hot to 1e-8: dS, dq and dk vanish and the
    backward checks nothing. So the u of a (sample, head) share a direction d (70 % of their energy): the other keys then
    score 22.4 +- 1.2, the best of them about 6 below the matching key: P is 0.9 to 0.99 on one key and 1e-2 to 1e-4 on
    the runners-up, the running maximum sits near 30, and dS is small but far from zero on every row."""
    w = randn(B, S, NH, 64, seed=seed)
    d = randn(B, 1, NH, 64, seed=seed + 4)
    u = 0.3 ** 0.5 * w + 0.7 ** 0.5 * 8.0 * torch.nn.functional.normalize(d, dim=-1)
    k = randn(B, S, NH, 64, seed=seed + 1)
    v = randn(B, S, NH, 64, seed=seed + 2)
    noise = randn(B, S, NH, 64, seed=seed + 3)
    for b, n in enumerate(lens):
        r = torch.arange(n)
        k[b, (r * 37) % n] = u[b, r] + 0.3 * noise[b, r]
    return torch.stack([4.0 * u, k, v], dim=2).reshape(B * S, 3 * NH * 64)


# name -> (B, S, NH, lengths, builder of the fp32 inputs)
CASES = {
    "edges": (15, 256, 2, EDGES, lambda *a: plain_inputs(*a, seed=101)),
    "tail130": (3, 130, 2, [130, 129, 2], lambda *a: plain_inputs(*a, seed=102)),
    "tail40": (3, 40, 2, [40, 33, 7], lambda *a: plain_inputs(*a, seed=103)),
    "tail600": (2, 600, 2, [600, 513], lambda *a: plain_inputs(*a, seed=104)),
    "sharp": (2, 256, 2, [256, 193], lambda *a: sharp_inputs(*a, seed=105)),
    "flat": (2, 256, 2, [256, 193], lambda *a: plain_inputs(*a, seed=109, qscale=0.02)),
    "heads": (2, 130, 3, [130, 65], lambda *a: plain_inputs(*a, seed=110, head_scales=[0.25, 1.0, 3.0])),
}
COMPACT = (5, 256, 2, [256, 200, 256, 256, 129], [70, 0, 33, 128, 129])

_REFS = {}   # case -> inputs, float64 reference and rounding model: evaluated once, shared by both forms, never modified


def reference(name):
    if name not in _REFS:
        if name == "compact":
            B, S, NH, lens, counts = COMPACT
            qkv = plain_inputs(B, S, NH, lens, seed=111).to(torch.bfloat16).to(DEV)
            g = torch.Generator().manual_seed(5)
            rows, off = [], [0]
            for b, n in enumerate(counts):
                rows += (torch.randperm(lens[b], generator=g)[:n].sort().values + b * S).tolist()
                off.append(off[-1] + n)
            rows_t = torch.tensor(rows, dtype=torch.int64, device=DEV)
            qoff = torch.tensor(off, dtype=torch.int32, device=DEV)
            q = qkv[rows_t, :NH * 64].contiguous()
            dctx = randn(off[-1], NH * 64, seed=112).to(torch.bfloat16).to(DEV)
            extra = {"q": q, "qoff": qoff, "rows": rows_t, "counts": counts}
        else:
            B, S, NH, lens, build = CASES[name]
            qkv = build(B, S, NH, lens).to(torch.bfloat16).to(DEV)
            q = qoff = None
            extra = {}
        H = NH * 64
        lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
        inside = (torch.arange(S, device=DEV)[None, :] < lengths[:, None]).reshape(B * S)
        if name != "compact":   # dO is zero on padded queries, as in the model (no loss there)
            dctx = (randn(B * S, H, seed=200 + list(CASES).index(name)).to(DEV) * inside[:, None]).to(torch.bfloat16)
        ref, mod = {}, {}
        for out, fn in ((ref, attention_fp64), (mod, attention_rounded)):
            out["ctx"], out["lse"], grad = fn(qkv, lengths, B, S, NH, q=q, qoff=qoff)
            out["dq"], out["dk"], out["dv"], _ = grad(dctx)
        _REFS[name] = dict(extra, B=B, S=S, NH=NH, lens=lens, qkv=qkv, lengths=lengths, inside=inside, dctx=dctx, ref=ref,
                           mod=mod)
    return _REFS[name]


def report(name, form, figures):
    line = f"rows {name:8s} form {form}:" + "".join(f"  {k} model {v['model']:.3e} kernel {v['got']:.3e}" for k, v in figures.items())
    print(line)


def case_forms():
    """Every case in both forced forms; the single-kernel form takes S <= 512, so its parameter is skipped above that."""
    out = []
    for n, c in CASES.items():
        too_long = [pytest.mark.skip(reason="the single-kernel form takes S <= 512")] if c[1] > 512 else []
        out += [pytest.param(n, 1, marks=too_long, id=f"{n}-1"), pytest.param(n, 0, id=f"{n}-0")]
    return out


@pytest.mark.parametrize("name,bwd_form", case_forms(), indirect=["bwd_form"])
def test_attention_rows(name, bwd_form):
    """Forward and backward of one case in one forced form (see the module docstring for the contract and the figures)."""
    L = _lib.lib()
    c = reference(name)
    B, S, NH, lens = c["B"], c["S"], c["NH"], c["lens"]
    H = NH * 64
    ref, mod = c["ref"], c["mod"]
    p, ctx, lse = attn_args(c["qkv"], c["lengths"], B, S, NH)
    assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 0
    delta = torch.zeros((B, NH, S), dtype=torch.float32, device=DEV)
    dqkv = torch.full((B * S, 3 * H), 7.0, dtype=torch.bfloat16, device=DEV)
    p.dctx, p.lddctx, p.delta, p.dqkv, p.lddqkv = c["dctx"].data_ptr(), H, delta.data_ptr(), dqkv.data_ptr(), 3 * H
    assert L.plb_launch_attn_bwd(C.byref(p), stream()) == 0
    torch.cuda.synchronize()
    n1 = sum(1 for n in lens if n == 1) * NH   # one valid key: P = 1, dP - delta = 0, so dq = dk = 0 in the reference
    fig = {}
    # ctx of padded query rows is computed like any other row (the weight-gradient GEMMs sum over them): same bound
    fig["ctx"] = check_rows("ctx", ctx, ref["ctx"], mod["ctx"], NH)
    fig["dq"] = check_rows("dq", dqkv[:, :H], ref["dq"], mod["dq"], NH, valid=c["inside"], n_abs=n1)
    fig["dk"] = check_rows("dk", dqkv[:, H:2 * H], ref["dk"], mod["dk"], NH, valid=c["inside"], n_abs=n1)
    fig["dv"] = check_rows("dv", dqkv[:, 2 * H:], ref["dv"], mod["dv"], NH, valid=c["inside"])
    report(name, bwd_form, fig)
    # the kernels keep MINUS the log-sum-exp in units of raw scores
    assert float((-lse.double() * ATTN_SCALE - ref["lse"]).abs().max()) <= 2e-3
    if bwd_form == 0:   # the single-kernel form keeps delta in LDS
        check_delta(delta, *attention_delta_terms(c["dctx"], ctx, B, S, NH))


@pytest.mark.parametrize("bwd_form", [0], indirect=True)
def test_attention_rows_compact_queries(bwd_form):
    """Compact-query mode (PlbAttn.qoff; two-kernel form only): ctx, dq, lse and delta by compact row; dk and dv of every
    key against the reference that sums over the compact queries alone. A sample without a query gets exactly zero dk / dv
    (nothing is summed), so its keys are held to exact zero like padded keys instead of falling under the absolute check."""
    L = _lib.lib()
    c = reference("compact")
    B, S, NH, Nq = c["B"], c["S"], c["NH"], int(c["qoff"][-1])
    H = NH * 64
    ref, mod = c["ref"], c["mod"]
    p, _, _ = attn_args(c["qkv"], c["lengths"], B, S, NH)
    ctx = torch.zeros((Nq, H), dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros((NH, Nq), dtype=torch.float32, device=DEV)
    delta = torch.zeros((NH, Nq), dtype=torch.float32, device=DEV)
    dq = torch.full((Nq, H), 5.0, dtype=torch.bfloat16, device=DEV)
    dqkv = torch.full((B * S, 3 * H), 7.0, dtype=torch.bfloat16, device=DEV)
    p.ctx, p.ldctx, p.lse = ctx.data_ptr(), H, lse.data_ptr()
    p.qoff, p.q, p.ldq, p.nq_total = c["qoff"].data_ptr(), c["q"].data_ptr(), H, Nq
    assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 0
    p.dctx, p.lddctx, p.dq, p.lddq = c["dctx"].data_ptr(), H, dq.data_ptr(), H
    p.delta, p.dqkv, p.lddqkv = delta.data_ptr(), dqkv.data_ptr(), 3 * H
    assert L.plb_launch_attn_bwd(C.byref(p), stream()) == 0
    torch.cuda.synchronize()
    has_q = torch.tensor(c["counts"], device=DEV).repeat_interleave(S) > 0
    keys = c["inside"] & has_q
    fig = {}
    fig["ctx"] = check_rows("ctx", ctx, ref["ctx"], mod["ctx"], NH)
    fig["dq"] = check_rows("dq", dq, ref["dq"], mod["dq"], NH)
    fig["dk"] = check_rows("dk", dqkv[:, H:2 * H], ref["dk"], mod["dk"], NH, valid=keys)
    fig["dv"] = check_rows("dv", dqkv[:, 2 * H:], ref["dv"], mod["dv"], NH, valid=keys)
    report("compact", bwd_form, fig)
    assert (dqkv[:, :H] == 7.0).all()   # the Q block of dqkv is not touched in compact mode
    assert float((-lse.double() * ATTN_SCALE - ref["lse"]).abs().max()) <= 2e-3
    check_delta(delta, *attention_delta_terms(c["dctx"], ctx, B, S, NH, c["qoff"]))
