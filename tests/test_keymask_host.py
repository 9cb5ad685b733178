"""No GPU: what the key-mask tests stand on, checked on the CPU.

  * keymask_ref.attention_fp64 / attention_rounded with a PREFIX mask are gpu_util's evaluations on the lengths, bit for bit;
  * with holes, the fp64 form is a float64 torch softmax with a -inf bias on the masked keys, and its gradients are autograd's;
  * gpu_util.check_rows catches ONE masked key leaking into ONE query row, a defect the aggregate limits of
    test_gpu_kernels.py (rel_l2 < 6e-3 for ctx, < 1.5e-2 for dq) let pass;
  * the word layout (keymask_ref.key_words_np: the spec of csrc/key_mask.hip) on hand-made rows;
  * the host's reading of a mask (plbert_amd.model._extent_from_mask / _lengths_and_key_mask);
  * oracle.albert_np.encoder_forward under a left-pad and a holes mask against transformers.AlbertModel (eager, fp32;
    tests/golden/keymask_h128.npz, captured by tools/capture_keymask_golden.py), 1e-5 abs below the extent.
"""
import os

import numpy as np
import pytest
import torch

import keymask_ref as R
import plbert_amd
from gpu_util import attention_fp64, attention_rounded, check_rows, rel_l2
from oracle import albert_np as onp
from plbert_amd.model import _extent_from_mask, _lengths_and_key_mask

B, S, NH = 2, 65, 1
H = NH * 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keymask_h128.npz")


def _inputs(seed, lens):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3 * H, generator=g).to(torch.bfloat16)
    lengths = torch.tensor(lens, dtype=torch.int32)
    inside = (torch.arange(S)[None, :] < lengths[:, None]).reshape(B * S)
    dctx = (torch.randn(B * S, H, generator=g) * inside[:, None]).to(torch.bfloat16)
    return qkv, lengths, inside, dctx


@pytest.mark.parametrize("with_lengths", [True, False])
def test_prefix_mask_equals_the_lengths_form(with_lengths):
    qkv, lengths, inside, dctx = _inputs(311, [65, 40])
    mask = inside.reshape(B, S).to(torch.int32)
    for mine, theirs in ((R.attention_fp64, attention_fp64), (R.attention_rounded, attention_rounded)):
        a = mine(qkv, mask, lengths if with_lengths else None, B, S, NH)
        b = theirs(qkv, lengths, B, S, NH)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for x, y in zip(a[2](dctx), b[2](dctx)):
            assert torch.equal(x, y)


def _holes_case():
    qkv, lengths, inside, dctx = _inputs(312, [65, 50])
    mask = inside.reshape(B, S).to(torch.int32).clone()
    mask[0, [0, 31, 32, 64]] = 0          # extent of sample 0 becomes 64
    mask[1, 10:20] = 0
    ext = R.extents(mask).to(torch.int32)
    assert ext.tolist() == [64, 50]
    inside = (torch.arange(S)[None, :] < ext[:, None]).reshape(B * S)
    dctx = dctx * inside[:, None]
    return qkv, mask, ext, inside, dctx


def test_holes_equal_a_torch_softmax_with_a_minus_inf_bias_and_autograd():
    qkv, mask, ext, inside, dctx = _holes_case()
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = [t.reshape(B, S, NH, 64).transpose(1, 2) for t in x.split(H, dim=1)]
    bias = torch.zeros(B, 1, 1, S, dtype=torch.float64).masked_fill(~R.valid_keys(mask, ext, S)[:, None, None, :], float("-inf"))
    s = (q @ k.transpose(2, 3)) * 0.125 + bias
    ctx = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B * S, H)
    (g,) = torch.autograd.grad(ctx, x, dctx.double())
    mine_ctx, mine_lse, grad = R.attention_fp64(qkv, mask, ext, B, S, NH)
    dq, dk, dv, _ = grad(dctx)
    assert torch.allclose(mine_ctx, ctx.detach(), rtol=0, atol=1e-12)
    assert torch.allclose(mine_lse, torch.logsumexp(s, dim=-1).detach(), rtol=0, atol=1e-12)
    assert torch.allclose(torch.cat([dq, dk, dv], dim=1), g, rtol=0, atol=1e-12)
    keys = R.valid_keys(mask, ext, S).reshape(B * S)
    assert not bool(dk[~keys].any()) and not bool(dv[~keys].any())          # a masked key receives no gradient as a key
    assert bool(dq[inside & ~keys].any())                                   # ... and a hole is still a query
    pr = R.probs_fp64(qkv, mask, ext, B, S, NH)
    assert torch.allclose(pr, torch.softmax(s, dim=-1).detach(), rtol=0, atol=1e-14)
    assert not bool(pr[~keys.reshape(B, S)[:, None, None, :].expand_as(pr)].any())


def test_one_leaking_key_is_caught_by_rows_and_missed_by_the_aggregate():
    """The planted defect: ONE query row of sample 1 is evaluated with ONE masked key (a hole) taking part — what a wrong bit
    index in one register of the masked kernels would do. The row is the typical one: the query for which that key would
    have the median probability (0.7 % among 90 valid keys: ctx of that row is off by 5 % of its norm, dq by 2 %. At 190
    valid keys the median key's 0.3 % still shows in ctx, 3.6 %, and no longer in dq: 1.2 % against a bound of 1.3 %)."""
    Bk, Sk, KEY = 2, 128, 55
    g = torch.Generator().manual_seed(313)
    qkv = torch.randn(Bk * Sk, 3 * H, generator=g).to(torch.bfloat16)
    mask = torch.ones(Bk, Sk, dtype=torch.int32)
    mask[0, [0, 63, 64]] = 0
    mask[1, 50:60] = 0
    mask[1, 100:] = 0
    ext = R.extents(mask).to(torch.int32)
    assert ext.tolist() == [128, 100]
    inside = (torch.arange(Sk)[None, :] < ext[:, None]).reshape(Bk * Sk)
    dctx = (torch.randn(Bk * Sk, H, generator=g) * inside[:, None]).to(torch.bfloat16)
    ref, mod = {}, {}
    for out, fn in ((ref, R.attention_fp64), (mod, R.attention_rounded)):
        out["ctx"], _, grad = fn(qkv, mask, ext, Bk, Sk, NH)
        out["dq"] = grad(dctx)[0]
    leak = mask.clone()
    leak[1, KEY] = 1
    x = qkv[Sk:].double()
    s = (x[:, :H] @ x[:, H:2 * H].T * 0.125).masked_fill(~R.valid_keys(leak, ext, Sk)[1][None, :], float("-inf"))
    p_leak = torch.softmax(s, dim=-1)[:ext[1], KEY]
    row = Sk + int(p_leak.argsort()[len(p_leak) // 2])
    ctx_l, _, grad_l = R.attention_rounded(qkv, leak, ext, Bk, Sk, NH)
    for name, t, limit in (("ctx", ctx_l, 6e-3), ("dq", grad_l(dctx)[0], 1.5e-2)):
        valid = None if name == "ctx" else inside
        check_rows(name, mod[name], ref[name], mod[name], NH, valid=valid)       # the model passes its own bound
        got = mod[name].clone()
        got[row] = t[row]
        with pytest.raises(AssertionError, match=rf"{name}: row {row} head 0 "):
            check_rows(name, got, ref[name], mod[name], NH, valid=valid)
        agg = rel_l2(got, ref[name])
        print(f"host keymask {name}: key of probability {float(p_leak[row - Sk]):.3e} leaked into row {row}: caught; "
              f"aggregate {agg:.3e} < {limit:g}")
        assert agg < limit


def test_word_layout():
    """Bit j & 31 of word j >> 5; two words per 64-key tile, whatever S; bits at or past the length, and past S, clear."""
    assert [R.row_stride(s) for s in (1, 64, 65, 128, 130, 2048)] == [2, 2, 4, 4, 6, 64]
    m = np.zeros((3, 70), np.int32)
    m[0, [0, 31, 32, 63, 64, 69]] = 1
    m[1, :] = 7                       # any nonzero value
    m[2, :] = 1
    w = R.key_words_np(m, [70, 70, 33], 70)
    assert w.dtype == np.uint32 and w.shape == (3, 4)
    assert w[0].tolist() == [0x80000001, 0x80000001, 0x00000021, 0]
    assert w[1].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0x0000003F, 0]
    assert w[2].tolist() == [0xFFFFFFFF, 0x00000001, 0, 0]
    assert R.key_words_np(m, None, 70)[2].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0x0000003F, 0]
    assert R.key_words_np(m[:, :64], [0, 64, 64], 64, ldkw=5)[0].tolist() == [1, 0, 0, 0, 0]      # length 0 reads as 1
    # the round trip: bit (j & 31) of word (j >> 5) is valid_keys
    g = torch.Generator().manual_seed(3)
    mask = (torch.rand(4, 130, generator=g) < 0.5).to(torch.int32)
    lens = torch.tensor([130, 129, 64, 1], dtype=torch.int32)
    w = R.key_words_np(mask.numpy(), lens.numpy(), 130)
    j = np.arange(130)
    bits = (w[:, j >> 5] >> (j & 31).astype(np.uint32)) & 1
    assert np.array_equal(bits.astype(bool), R.valid_keys(mask, lens, 130).numpy())


def test_extent_and_prefix_from_a_mask():
    am = torch.tensor([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1], [2, 0, 0, 0, 0]])
    ext, prefix = _extent_from_mask(am)
    assert ext.dtype == torch.int32 and ext.tolist() == [3, 5, 1] and prefix is True
    assert _lengths_and_key_mask(None) == (None, None)
    lengths, km = _lengths_and_key_mask(am)
    assert km is None and lengths.tolist() == [3, 5, 1]
    for bad, want in ((torch.tensor([[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]]), [5, 5]),        # left pad
                      (torch.tensor([[1, 0, 1, 0, 0], [1, 1, 0, 0, 0]]), [3, 2]),        # a hole
                      (torch.tensor([[0, 0, 0, 0, 1], [1, 0, 0, 0, 0]]), [5, 1])):       # a single key at the end
        ext, prefix = _extent_from_mask(bad)
        assert ext.tolist() == want and prefix is False
        lengths, km = _lengths_and_key_mask(bad)
        assert km is bad and lengths.tolist() == want
        assert ext.tolist() == R.extents(bad).tolist()
    for empty in (torch.tensor([[1, 1, 0], [0, 0, 0]]), torch.tensor([[0, 1, 0], [0, 0, 0]])):
        with pytest.raises(ValueError, match="no valid token"):
            _extent_from_mask(empty)
    with pytest.raises(ValueError, match=r"\[B,S\]"):
        _extent_from_mask(torch.ones(2, 3, 3))


def test_oracle_under_non_prefix_masks_against_transformers():
    """SURVEY §8(c)'s bound for the fp32 restatement, 1e-5 abs, at the positions below each row's extent (transformers leaves
    values at pad positions too; nothing reads them)."""
    g = np.load(GOLDEN)
    shape = dict(vocab_size=int(g["vocab_size"]), embedding_size=64, hidden_size=128, num_attention_heads=2,
                 intermediate_size=128, num_hidden_layers=2, max_position_embeddings=int(g["max_position_embeddings"]))
    cfg = onp.Config(**shape)
    # the fixture holds the generator's seed, not the weights (tools/capture_keymask_golden.py)
    P = plbert_amd.deterministic_state_dict(plbert_amd.AlbertConfig(**shape), shape["vocab_size"], seed=int(g["seed"]),
                                            scale=float(g["scale"]))
    for which in ("leftpad", "holes"):
        mask = g[f"mask_{which}"]
        hid, _ = onp.encoder_forward(cfg, P, g["ids"], mask, np.float32, keep=False)
        ext = R.extents(torch.as_tensor(mask)).numpy()
        below = np.arange(mask.shape[1])[None, :] < ext[:, None]
        err = np.abs(hid - g[f"hidden_{which}"])[below].max()
        print(f"oracle vs transformers, {which}: max abs {err:.3e}")
        assert err < 1e-5
    assert (g["mask_holes"][:, 0] == 0).any() and (g["mask_leftpad"][:, 0] == 0).all()
