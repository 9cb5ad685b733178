"""Host: the pooler backward's float64 restatement and error model (tests/pooler_ref.py), and the new rows of the binding and
entry tables against the headers. No GPU.

 - the restatement equals torch autograd in float64 on tanh(linear(h0, W, b)) to 1e-12;
 - the error model holds for a float32 numpy emulation of the kernels' sums (every element, none excluded), including
   saturated rows (y = +-1 in fp32: dpre exactly 0) and exact zeros in d_pooled;
 - plb_launch_pooler_bwd / plb_launch_seed_dy_first_rows / plb_encode_bwd_pooled are bound as the headers declare them, the
   rung is reached only with a d_pooled, and its argument names are the header's in order."""
import itertools

import numpy as np
import pytest
import torch

import c_header
import pooler_ref as R
from plbert_amd import _lib, build
from plbert_amd.engine import ENTRY_ARGS, POOLED_ENTRY_ARGS, encoder_entry


def _case(B, H, seed, kind="ordinary"):
    rng = np.random.default_rng(seed)
    h0 = R.bf16_round(rng.standard_normal((B, H)).astype(np.float32))
    W = (rng.standard_normal((H, H)) * 0.02).astype(np.float32)
    bias = (rng.standard_normal(H) * 0.02).astype(np.float32)
    dp = rng.standard_normal((B, H)).astype(np.float32)
    if kind == "saturated":
        bias[::2] = 40.0
        bias[1::4] = -40.0
    if kind == "zeros":
        dp[rng.random((B, H)) < 0.5] = 0.0
        dp[0] = 0.0
    return h0, W, bias, dp


@pytest.mark.parametrize("B, H", [(1, 64), (3, 128), (5, 192)])
def test_restatement_is_torch_autograd_in_float64(B, H):
    h0, W, bias, dp = (torch.from_numpy(x).double() for x in _case(B, H, 7))
    h0.requires_grad_(True); W.requires_grad_(True); bias.requires_grad_(True)
    y = torch.tanh(torch.nn.functional.linear(h0, W, bias))
    y.backward(dp)
    dpre, dW, db, dh0 = R.backward(h0.detach().numpy(), W.detach().numpy(), bias.detach().numpy(), dp.numpy())
    assert np.abs(R.forward(h0.detach().numpy(), W.detach().numpy(), bias.detach().numpy()) - y.detach().numpy()).max() <= 1e-12
    for got, want in ((dW, W.grad), (db, bias.grad), (dh0, h0.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-12
    assert np.abs(dpre - (dp * (1 - y.detach() ** 2)).numpy()).max() <= 1e-12


@pytest.mark.parametrize("kind", ["ordinary", "saturated", "zeros"])
@pytest.mark.parametrize("B, H", [(1, 128), (3, 128), (3, 256)])
def test_error_model_holds_for_an_fp32_emulation(B, H, kind):
    h0, W, bias, dp = _case(B, H, 11 + B + H, kind)
    y, dpre, dW, db, dh0 = R.fp32_emulation(h0, W, bias, dp)
    want = R.backward(h0, W, bias, dp, y=y)          # at the emulation's own y, as the GPU test takes plb_pooler's
    bound = R.bounds(h0, W, dp, y)
    for name, got, ref, e in zip(("dpre", "dW", "db", "dh0"), (dpre, dW, db, dh0), want, bound):
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= e).all(), (name, float((err - e).max()))
    if kind == "saturated":
        assert (np.abs(y[:, ::2]) == 1.0).all() and (dpre[:, ::2] == 0).all() and (dW[::2] == 0).all() and (db[::2] == 0).all()
    if kind == "zeros":
        assert (dpre[dp == 0] == 0).all() and not dh0[0].any()
    # the bound means something: a y that is off by 2^-20 (a tanh of another accuracy class, a bf16 operand) is outside it
    if kind == "ordinary":
        off = (y + np.float32(2.0 ** -20)).astype(np.float32)
        d2 = (dp * (np.float32(1) - off * off)).astype(np.float32)
        assert (np.abs(d2.astype(np.float64) - want[0]) > bound[0]).any()


def test_bf16_rounding_is_round_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 0.0], dtype=np.float32)   # ties at 1 + 2^-8, 1 + 3 * 2^-8
    assert R.bf16_round(x).tolist() == [1.0, 1.0, 1.015625, -1.0, 0.0]
    t = torch.from_numpy(np.random.default_rng(0).standard_normal(4096).astype(np.float32))
    assert np.array_equal(R.bf16_round(t.numpy()), t.bfloat16().float().numpy())


# ---- the new rows of the tables ---------------------------------------------------------------------------------------------
def test_launchers_are_bound_as_the_kernel_header_declares_them():
    hdr = c_header.kernels()
    mirrors = c_header.mirrors(_lib)
    for name in ("plb_launch_pooler_bwd", "plb_launch_seed_dy_first_rows"):
        assert name in hdr.protos and name in _lib.INTERNAL, name
        assert c_header.signature_mismatch(hdr, hdr.protos[name], *_lib.INTERNAL[name], mirrors) is None
    names = [p.name for p in hdr.protos["plb_launch_pooler_bwd"].params]
    assert names == ["hidden", "ldh", "rows", "B", "S", "H", "W", "bias", "d_pooled", "dpre", "dW", "db", "dh0", "stream"]
    assert "pooler_bwd.hip" in build.SOURCES


def test_entry_point_is_bound_and_is_a_superset_of_the_masked_rung():
    hdr = c_header.public()
    name = "plb_encode_bwd_pooled"
    assert name in _lib.PUBLIC and name not in ENTRY_ARGS
    assert c_header.signature_mismatch(hdr, hdr.protos[name], *_lib.PUBLIC[name], c_header.mirrors(_lib)) is None
    mine, masked = ([p.name for p in hdr.protos[n].params] for n in (name, "plb_encode_bwd_masked"))
    assert mine == masked[:-1] + ["d_pooled", "stream"]
    assert list(POOLED_ENTRY_ARGS[name]) == mine
    assert _lib.PUBLIC[name][1] == _lib.PUBLIC["plb_encode_bwd_masked"][1][:-1] + [_lib.vp, _lib.vp]


def test_the_rung_is_reached_only_with_a_d_pooled():
    for inputs, mask, below, want in itertools.product([False, True], repeat=4):
        args = ("encode_bwd", None, inputs, mask, [None] if below else None, want)
        assert encoder_entry(*args, d_pooled=True) == "plb_encode_bwd_pooled"
        assert encoder_entry(*args, d_pooled=False) == encoder_entry(*args) != "plb_encode_bwd_pooled"
    for family in ("forward", "encode"):
        assert "pooled" not in encoder_entry(family, True, True, True)
