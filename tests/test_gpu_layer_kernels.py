"""-m gpu: the two kernels of csrc/layer_outputs.hip through their launchers.

plb_launch_attn_probs: qkv from seeded normals (bf16), lse from plb_launch_attn_fwd on the same qkv; every element within
3e-3 * p_ref + 1e-30 of the float64 softmax of the same bf16 operands (tests/layer_outputs_ref.py). The 3e-3: 2e-3 is the
per-element bound tests/test_gpu_attention_rows.py holds the stored log-sum-exp to, and an error d of the log-sum-exp is a
relative error exp(d) - 1 of every probability of the row; the rest allows for the fp32 score (64 products) and the
hardware exponential, below 1e-4 for these inputs. Row sums within 3e-3 of 1, pad columns and pad query rows all-zero bytes,
the guard behind the output untouched, no element left unwritten, the packed layout bit-equal to the padded one. The rows
the kernel must not read (at or past a sample's length) hold NaN in the buffer it is given.

Measured on MI355X (printed per case by the first run: worst |p - p_ref| / p_ref over the elements with p_ref >= 1e-30, and
the worst |row sum - 1|):

    case     layout   worst relative   worst row sum
    edges    padded   1.310e-06        7.956e-07
    edges    packed   1.310e-06        7.956e-07
    odd37    padded   9.072e-07        5.438e-07
    tail40   padded   9.491e-07        6.089e-07

plb_launch_add_row_grad: bit-exact against (res.float() + g).to(bfloat16) on the value classes of test_gpu_encode.py's
_seed_values, NaN in g at pad positions never surfaces, every row in [0, Tp) written once, nothing behind Tp, refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import layer_outputs_ref as lref
from gpu_util import attn_args, stream
from plbert_amd import _lib
from plbert_amd.engine import packing_plan
from test_gpu_encode import K_SHAPE, _seed_values, _valid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 0.125

# name -> (B, S, NH, lengths): every edge of the 32-query wave, the 64-key tile and the 128-row tile as a length and a
# sequence that ends inside each; S odd (scalar stores, rows that start on no 16-byte boundary); S below one tile
PROB_CASES = {
    "edges": (11, 300, 2, [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300]),
    "odd37": (3, 37, 2, [37, 20, 1]),
    "tail40": (3, 40, 2, [40, 33, 7]),
}
_REF = {}


def _prob_case(name):
    """Inputs and float64 reference of one case: made once, shared by the layouts, never modified."""
    if name not in _REF:
        B, S, NH, lens = PROB_CASES[name]
        H = NH * 64
        g = torch.Generator().manual_seed(300 + len(name))
        qkv = torch.randn(B * S, 3 * H, generator=g).to(torch.bfloat16)
        x = qkv.float().reshape(B, S, 3, NH, 64)
        ref = lref.attn_probs_ref(x[:, :, 0].permute(0, 2, 1, 3).numpy(), x[:, :, 1].permute(0, 2, 1, 3).numpy(), lens, SCALE)
        _REF[name] = (qkv, torch.as_tensor(ref))
    return _REF[name]


def _launch_probs(qkv_fwd, qkv_probs, lens_d, row_start, B, S, NH, offset_floats=0):
    """lse from the attention forward on qkv_fwd (finite everywhere), probabilities from qkv_probs (NaN in the rows that must
    not be read). Returns (out [B,NH,S,S], guard, the whole buffer)."""
    L = _lib.lib()
    p, _, lse = attn_args(qkv_fwd, lens_d, B, S, NH)
    if row_start is not None:
        p.row_start = row_start.data_ptr()
    assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 0
    n = B * NH * S * S
    buf = torch.full((offset_floats + n + 64,), float("nan"), dtype=torch.float32, device=DEV)
    out = buf[offset_floats:offset_floats + n]
    assert L.plb_launch_attn_probs(qkv_probs.data_ptr(), qkv_probs.stride(0), lse.data_ptr(), lens_d.data_ptr(),
                                   None if row_start is None else row_start.data_ptr(), B, S, NH, SCALE, out.data_ptr(),
                                   stream()) == 0
    torch.cuda.synchronize()
    assert bool(buf[:offset_floats].isnan().all()) and bool(buf[offset_floats + n:].isnan().all())   # guards untouched
    return out.view(B, NH, S, S).cpu()


def _check_probs(name, layout, got, ref, lens, S):
    v = torch.as_tensor(_valid(lens, S))
    assert not bool(got.isnan().any()), "an element of the output was not written"
    rows = v[:, None, :, None].expand_as(got)
    cols = v[:, None, None, :].expand_as(got)
    assert not bool(got[~rows].view(torch.int32).any()) and not bool(got[~cols].view(torch.int32).any())   # all-zero bytes
    err = (got.double() - ref).abs()
    big = ref >= 1e-30
    worst = float((err[big] / ref[big]).max())
    sums = float((got.double().sum(-1)[v[:, None, :].expand(got.shape[:3])] - 1).abs().max())
    print(f"attn_probs {name} {layout}: worst relative {worst:.3e}  worst row sum {sums:.3e}")
    assert bool((err <= 3e-3 * ref + 1e-30).all()), (name, layout, worst)
    assert sums <= 3e-3, (name, layout, sums)


@pytest.mark.parametrize("name", sorted(PROB_CASES))
def test_attn_probs_against_float64(name):
    B, S, NH, lens = PROB_CASES[name]
    qkv, ref = _prob_case(name)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    v = torch.as_tensor(_valid(lens, S)).reshape(-1)
    padded = qkv.to(DEV)
    poisoned = padded.clone()
    poisoned[~v.to(DEV)] = float("nan")
    got = _launch_probs(padded, poisoned, lens_d, None, B, S, NH)
    _check_probs(name, "padded", got, ref, lens, S)
    if S % 4 == 0:   # an output that is not 16-byte aligned takes the scalar stores: the same bits
        shifted = _launch_probs(padded, poisoned, lens_d, None, B, S, NH, offset_floats=1)
        assert torch.equal(shifted.view(torch.int32), got.view(torch.int32))
    plan = packing_plan(lens, S).to(DEV, non_blocking=False)
    if not plan.packed:
        return
    pos, rows = lref.token_rows(lens, S, plan.row_start_host)
    pk_fwd = torch.randn(plan.rows, qkv.shape[1], generator=torch.Generator().manual_seed(9)).to(torch.bfloat16).to(DEV)
    pk_fwd[rows.to(DEV)] = padded[pos.to(DEV)]
    pk_probs = torch.full_like(pk_fwd, float("nan"))
    pk_probs[rows.to(DEV)] = padded[pos.to(DEV)]
    got_pk = _launch_probs(pk_fwd, pk_probs, lens_d, plan.row_start, B, S, NH)
    _check_probs(name, "packed", got_pk, ref, lens, S)
    assert torch.equal(got_pk.view(torch.int32), got.view(torch.int32))      # packed is bit-equal to padded


def test_attn_probs_without_lengths_and_refusals():
    L = _lib.lib()
    B, S, NH = 2, 40, 2
    qkv, _ = _prob_case("tail40")
    qkv = qkv[: B * S].contiguous().to(DEV)
    x = qkv.float().cpu().reshape(B, S, 3, NH, 64)
    ref = torch.as_tensor(lref.attn_probs_ref(x[:, :, 0].permute(0, 2, 1, 3).numpy(), x[:, :, 1].permute(0, 2, 1, 3).numpy(),
                                              [S] * B, SCALE))
    p, _, lse = attn_args(qkv, None, B, S, NH)
    assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 0
    out = torch.full((B, NH, S, S), float("nan"), device=DEV)
    args = lambda **kw: [kw.get("qkv", qkv.data_ptr()), kw.get("ld", 3 * NH * 64), kw.get("lse", lse.data_ptr()), None,
                         kw.get("row_start"), kw.get("B", B), kw.get("S", S), NH, SCALE, kw.get("out", out.data_ptr()), stream()]
    assert L.plb_launch_attn_probs(*args()) == 0
    torch.cuda.synchronize()
    assert bool(((out.cpu().double() - ref).abs() <= 3e-3 * ref + 1e-30).all())
    before = out.clone()
    for bad in (dict(qkv=None), dict(lse=None), dict(out=None), dict(B=0), dict(S=0), dict(ld=3 * NH * 64 - 8), dict(ld=3 * NH * 64 + 4),
                dict(qkv=qkv.data_ptr() + 2), dict(out=out.data_ptr() + 2), dict(row_start=lse.data_ptr())):   # (a plan needs lengths)
        assert L.plb_launch_attn_probs(*args(**bad)) != 0, bad
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), out.view(torch.int32))      # nothing was launched


# ---- add_row_grad -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["P", "K", "H768"])
def test_add_row_grad_is_bit_exact_and_writes_every_row_once(case):
    L = _lib.lib()
    if case == "P":
        B, S, H, lens, packed = 3, 40, 128, [40, 33, 7], False
    elif case == "K":
        (B, S, lens), H, packed = K_SHAPE, 128, True
    else:   # more than one pass of the grid, H no power of two, a tail of 116 rows behind B*S
        B, S, H, lens, packed = 2, 70, 768, [70, 3], False
    lens = np.asarray(lens, np.int32)
    valid = torch.as_tensor(_valid(lens, S))
    g = _seed_values(B * S * H, 17).view(B, S, H)
    g_clean = g.clone()
    g[~valid] = float("nan")           # never read: a NaN that reached the output would show below
    lens_d = torch.as_tensor(lens).to(DEV)
    if packed:
        plan = packing_plan(lens, S).to(DEV, non_blocking=False)
        assert plan.packed
        Tp, row_start, table = plan.rows, plan.row_start, plan.row_start_host
    else:
        Tp, row_start, table = (B * S + 127) // 128 * 128, None, None
    pos, rows = lref.token_rows(lens, S, table)
    # res: finite bf16 values of every size class (so that no sum is a NaN, whose bits would not be comparable), -0 included
    res = (_seed_values(Tp * H, 18).clamp(-1e30, 1e30)).view(Tp, H).to(torch.bfloat16)
    want = lref.add_row_grad_ref(res, g_clean, pos, rows)
    buf = torch.full((Tp + 8, H), -1.5, dtype=torch.bfloat16, device=DEV)   # sentinel (0xBFC0), 8 guard rows behind Tp
    sentinel = int(buf[0, 0].view(torch.int16))
    res_d, g_d = res.to(DEV), g.to(DEV)
    rs = None if row_start is None else row_start.data_ptr()
    assert L.plb_launch_add_row_grad(res_d.data_ptr(), g_d.data_ptr(), lens_d.data_ptr(), rs, B, S, H, Tp, buf.data_ptr(),
                                     stream()) == 0
    torch.cuda.synchronize()
    got = buf.cpu().view(torch.int16)
    assert torch.equal(got[:Tp], want.view(torch.int16))     # rows of valid positions: the sum; every other row: res itself
    assert not torch.equal(want[rows], res[rows])            # (the sum is not the operand: the check above is not vacuous)
    assert bool((got[Tp:] == sentinel).all())                # nothing behind row Tp was written
    assert torch.equal(res_d.cpu().view(torch.int16), res.view(torch.int16))   # the operand is left alone
    # in place (out == res) gives the same rows
    inplace = res_d.clone()
    assert L.plb_launch_add_row_grad(inplace.data_ptr(), g_d.data_ptr(), lens_d.data_ptr(), rs, B, S, H, Tp, inplace.data_ptr(),
                                     stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(inplace.cpu().view(torch.int16), want.view(torch.int16))
    # lengths == NULL (padded only): every position is valid
    if not packed:
        g2 = torch.nan_to_num(g_d, nan=0.25)
        assert L.plb_launch_add_row_grad(res_d.data_ptr(), g2.data_ptr(), None, None, B, S, H, Tp, buf.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        full = (res[: B * S].float() + g2.cpu().view(B * S, H)).to(torch.bfloat16)
        assert torch.equal(buf[: B * S].cpu().view(torch.int16), full.view(torch.int16))
        assert torch.equal(buf[B * S:Tp].cpu().view(torch.int16), res[B * S:].view(torch.int16))
    # bad arguments are refused before any launch
    before = buf.clone()
    a = (res_d.data_ptr(), g_d.data_ptr(), lens_d.data_ptr(), None, B, S, H, Tp, buf.data_ptr(), stream())
    bad = lambda i, v: a[:i] + (v,) + a[i + 1:]
    for args in (bad(7, B * S - 1), bad(1, g_d.data_ptr() + 4), bad(0, None), bad(1, None), bad(8, None), bad(6, H + 2),
                 bad(0, res_d.data_ptr() + 2), bad(3, lens_d.data_ptr())[:2] + (None,) + bad(3, lens_d.data_ptr())[3:]):
        assert L.plb_launch_add_row_grad(*args) != 0
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int16), buf.view(torch.int16))
