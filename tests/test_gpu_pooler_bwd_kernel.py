"""The pooler backward at kernel level (-m gpu; csrc/pooler_bwd.hip): plb_launch_pooler_bwd and plb_launch_seed_dy_first_rows
called directly, against the float64 restatement and the error model of tests/pooler_ref.py.

Shapes: H in {128, 768, 1024} (one, three and four passes of a wave over a row), B in {1, 3}, the samples' rows scattered
through a larger bf16 matrix by a row table (and once without one: rows b*S). Values: ordinary; rows of W and bias that drive
|pre| far enough that y = +-1 in fp32 (dpre then exactly 0); d_pooled with exact zeros.
Checks: every element of dpre, dW, db and dh0 within its bound of the restatement taken at y = the bits plb_launch_pooler
returns on the fp32 image of the same rows (no element is excluded); guard elements around every output untouched; two runs
bitwise equal; the seeded rows of dy are bf16(d_hidden + dh0) exactly and no other row of dy is written."""
import numpy as np
import pytest
import torch

import pooler_ref as R
from gpu_util import stream
from plbert_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case(B, H, kind, seed):
    g = np.random.default_rng(seed)
    rows_total, ld = 9, H + 8
    hid = R.bf16_round(g.standard_normal((rows_total, ld)).astype(np.float32) * 1.5)
    rows = np.array([5, 0, 7][:B], dtype=np.int32)
    W = (g.standard_normal((H, H)) * H ** -0.5).astype(np.float32)
    bias = (g.standard_normal(H) * 0.2).astype(np.float32)
    dp = g.standard_normal((B, H)).astype(np.float32)
    if kind == "saturated":
        bias[::2] = 60.0
        bias[1::4] = -60.0
    if kind == "zeros":
        dp[g.random((B, H)) < 0.5] = 0.0
        dp[B - 1] = 0.0
    return hid, ld, rows, W, bias, dp


def _launch(hid, ld, rows, S, W, bias, dp):
    """One plb_launch_pooler on the fp32 image + one plb_launch_pooler_bwd; device tensors with 4 guard floats at each end."""
    L = _lib.lib()
    B, H = dp.shape
    hb = torch.from_numpy(hid).to(DEV).bfloat16().contiguous()
    assert torch.equal(hb.float().cpu(), torch.from_numpy(hid))                     # the case IS bf16 values
    rd = None if rows is None else torch.from_numpy(rows).to(DEV)
    Wd, bd, dpd = (torch.from_numpy(x).to(DEV) for x in (W, bias, dp))
    first = np.arange(B) * S if rows is None else rows
    h0 = hid[first][:, :H]
    # plb_pooler's bits: the forward launch on an fp32 [B,1,H] image of the same rows
    y = torch.empty(B, H, device=DEV)
    assert L.plb_launch_pooler(torch.from_numpy(np.ascontiguousarray(h0)).to(DEV).data_ptr(), B, 1, H, Wd.data_ptr(), bd.data_ptr(),
                               y.data_ptr(), stream()) == 0
    G = 4   # guard floats (keeps dW 16-byte aligned)
    outs = [torch.full((n + 2 * G,), 7.0, device=DEV) for n in (B * H, H * H, H, B * H)]
    assert L.plb_launch_pooler_bwd(hb.data_ptr(), ld, None if rd is None else rd.data_ptr(), B, S, H, Wd.data_ptr(), bd.data_ptr(),
                                   dpd.data_ptr(), *[o[G:].data_ptr() for o in outs], stream()) == 0
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o[:G] == 7.0).all()) and bool((o[-G:] == 7.0).all())
    dpre, dW, db, dh0 = (o[G:-G].cpu().numpy() for o in outs)
    return h0, y.cpu().numpy(), dpre.reshape(B, H), dW.reshape(H, H), db, dh0.reshape(B, H)


@pytest.mark.parametrize("kind", ["ordinary", "saturated", "zeros"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [128, 768, 1024])
def test_every_element_is_within_its_bound_and_runs_are_bitwise_equal(H, B, kind):
    hid, ld, rows, W, bias, dp = _case(B, H, kind, 100 * H + 10 * B + len(kind))
    h0, y, *got = _launch(hid, ld, rows, 3, W, bias, dp)
    want = R.backward(h0, W, bias, dp, y=y)
    bound = R.bounds(h0, W, dp, y)
    assert np.abs(y.astype(np.float64) - R.forward(h0, W, bias)).max() <= 1e-5      # (and y is the pooler's output)
    for name, a, ref, e in zip(("dpre", "dW", "db", "dh0"), got, want, bound):
        err = np.abs(a.astype(np.float64) - ref)
        print(f"{name}: max err {err.max():.3e}, max bound {e.max():.3e}, worst err/bound "
              f"{(err / np.where(e > 0, e, np.inf)).max():.3f}, elements {err.size}")
        assert (err <= e).all(), (name, int((err > e).sum()), float((err - e).max()))
    if kind == "saturated":
        assert (np.abs(y[:, ::2]) == 1.0).all() and (np.abs(y[:, 1::4]) == 1.0).all()
        assert (got[0][:, ::2] == 0).all() and (got[0][:, 1::4] == 0).all() and (got[1][::2] == 0).all() and (got[2][::2] == 0).all()
    if kind == "zeros":
        assert (got[0][dp == 0] == 0).all() and not got[3][B - 1].any()
    again = _launch(hid, ld, rows, 3, W, bias, dp)
    for a, b in zip(got, again[2:]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_without_a_row_table_sample_b_is_row_b_times_s():
    B, H, S = 3, 128, 4
    hid, ld, _, W, bias, dp = _case(B, H, "ordinary", 5)
    hid = np.concatenate([hid, hid[::-1]])[: B * S]                                  # 12 rows: samples at rows 0, 4, 8
    a = _launch(hid, ld, None, S, W, bias, dp)
    b = _launch(hid, ld, np.array([0, 4, 8], dtype=np.int32), S, W, bias, dp)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("with_d_hidden", [True, False])
@pytest.mark.parametrize("packed", [True, False])
def test_first_rows_of_dy_are_one_add_and_one_rounding(packed, with_d_hidden):
    L = _lib.lib()
    B, S, H, Tp = 3, 5, 128, 384
    g = np.random.default_rng(3)
    dh0 = g.standard_normal((B, H)).astype(np.float32)
    dh0[0, :3] = [0.0, -0.0, 1.00390625]
    dhid = g.standard_normal((B, S, H)).astype(np.float32)
    rows = np.array([0, 128, 256], dtype=np.int32) if packed else None
    dy = torch.full((Tp, H), 3.0, device=DEV).bfloat16()
    before = dy.clone()
    dhid_d, dh0_d = torch.from_numpy(dhid).to(DEV), torch.from_numpy(dh0).to(DEV)
    rd = torch.from_numpy(rows).to(DEV) if packed else None
    assert L.plb_launch_seed_dy_first_rows(dhid_d.data_ptr() if with_d_hidden else None, dh0_d.data_ptr(),
                                           rd.data_ptr() if packed else None, B, S, H, dy.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    first = rows if packed else np.arange(B) * S
    want = (dhid_d[:, 0] + dh0_d) if with_d_hidden else (torch.zeros_like(dh0_d) + dh0_d)
    assert torch.equal(dy[first.tolist()].view(torch.int16), want.bfloat16().view(torch.int16))
    keep = torch.ones(Tp, dtype=torch.bool, device=DEV)
    keep[first.tolist()] = False
    assert torch.equal(dy[keep].view(torch.int16), before[keep].view(torch.int16))


def test_launchers_refuse_what_they_cannot_run():
    L = _lib.lib()
    t = torch.zeros(2 * 128 * 128, device=DEV)   # (every operand of the one launch that runs fits: dW is 128 x 128 floats)
    p = t.data_ptr()
    ok = (p, 128, None, 1, 1, 128, p, p, p, p, p, p, p)
    assert L.plb_launch_pooler_bwd(*ok, stream()) == 0
    assert L.plb_launch_pooler_bwd(None, *ok[1:], stream()) != 0                    # no hidden rows
    assert L.plb_launch_pooler_bwd(p, 64, *ok[2:], stream()) != 0                   # row stride below H
    assert L.plb_launch_pooler_bwd(*ok[:5], 96, *ok[6:], stream()) != 0             # H no multiple of 64
    assert L.plb_launch_pooler_bwd(*ok[:8], p + 4, *ok[9:], stream()) != 0          # misaligned d_pooled
    assert L.plb_launch_seed_dy_first_rows(None, p + 4, None, 1, 1, 128, p, stream()) != 0
    assert L.plb_launch_seed_dy_first_rows(None, None, None, 1, 1, 128, p, stream()) != 0
    torch.cuda.synchronize()
