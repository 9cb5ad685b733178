"""Key masks (PlbAttn.key_words; include/plbert.h: plb_*_masked) restated for the tests: nothing here calls a kernel.

  attention_fp64 / attention_rounded   gpu_util's two evaluations with the valid keys taken from a [B,S] mask instead of a
                                       length alone, under the same rounding model (gpu_util.attention_rounded's docstring)
  key_words_np                         the word layout in numpy: THE SPEC of the bit order and of the row stride
  extents / valid_keys                 the extent of a mask row and the keys that take part

The rule is transformers' 2-D key-padding rule: key j of sample b takes part in the softmax of every query of b iff
mask[b,j] != 0 (and j lies below the sample's length). A masked key below the length — a hole — is still a query.
"""
import numpy as np
import torch

from gpu_util import ATTN_SCALE, _r16


def extents(mask):
    """1 + the last position with a nonzero entry, per row (0 for a row without one). mask [B,S], torch."""
    m = mask != 0
    S = m.shape[1]
    return (m * torch.arange(1, S + 1, device=m.device)[None, :]).amax(dim=1)


def valid_keys(mask, lengths, S):
    """bool [B,S]: the keys that take part — mask != 0 below the length as the kernels read it (clamped to [1, S])."""
    m = mask != 0
    if lengths is None:
        return m
    lens = lengths.long().clamp(1, S)
    return m & (torch.arange(S, device=m.device)[None, :] < lens[:, None])


def row_stride(S):
    """Words per row: every 64-key tile owns two whole words."""
    return 2 * ((S + 63) // 64)


def key_words_np(mask, lengths, S, ldkw=None):
    """uint32 [B, ldkw]: bit j & 31 of word j >> 5 of row b is key j of sample b; bits at or past the length are clear, and
    so are the bits of the keys past S in the row's last words. mask: [B,S] integers (numpy), lengths: [B] or None."""
    mask = np.asarray(mask)
    B = mask.shape[0]
    ldkw = row_stride(S) if ldkw is None else ldkw
    lens = np.full(B, S) if lengths is None else np.clip(np.asarray(lengths), 1, S)
    out = np.zeros((B, ldkw), dtype=np.uint32)
    for b in range(B):
        for j in range(S):
            if j < lens[b] and mask[b, j] != 0:
                out[b, j >> 5] |= np.uint32(1) << np.uint32(j & 31)
    return out


def _attention_eval(qkv, valid, B, S, NH, rounded):
    """gpu_util._attention_eval (full queries) with `valid` [B,S] bool in the place of `key < length`."""
    H = NH * 64
    x = qkv.double()
    heads = lambda t: t.reshape(B, S, NH, 64).permute(0, 2, 1, 3)          # [B*S, H] -> [B, NH, S, 64]
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B * S, H)
    Q, K, V = heads(x[:, :H]), heads(x[:, H:2 * H]), heads(x[:, 2 * H:3 * H])
    masked = ~valid[:, None, None, :]
    sraw = Q @ K.transpose(2, 3)
    s = (sraw * ATTN_SCALE).masked_fill(masked, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    lse = (m + torch.log(l)).squeeze(-1)
    ctx = _r16((_r16(e) @ V) / l) if rounded else (e / l) @ V

    def grad(dctx):
        dO = heads(dctx.double())
        if rounded:
            lse_st = (-lse / ATTN_SCALE).float().double()
            P = torch.exp((sraw + lse_st[..., None]) * ATTN_SCALE).masked_fill(masked, 0.0)
        else:
            P = e / l
        delta = (dO * ctx).sum(-1, keepdim=True)
        dS = P * (dO @ V.transpose(2, 3) - delta)
        if rounded:
            dS = _r16(dS)
        dq = (dS @ K) * ATTN_SCALE
        dk = (dS.transpose(2, 3) @ Q) * ATTN_SCALE
        dv = (_r16(P) if rounded else P).transpose(2, 3) @ dO
        if rounded:
            dq, dk, dv = _r16(dq), _r16(dk), _r16(dv)
        return rows(dq), rows(dk), rows(dv), -delta.squeeze(-1)

    return rows(ctx), lse, grad


def attention_fp64(qkv, mask, lengths, B, S, NH):
    """float64 attention on the (bf16-rounded) inputs with the keys of valid_keys(mask, lengths, S): ctx [B*S, H], lse
    [B, NH, S] (natural log, scaled scores), grad(dctx) -> (dq, dk, dv, delta), as gpu_util.attention_fp64."""
    return _attention_eval(qkv, valid_keys(mask, lengths, S), B, S, NH, False)


def attention_rounded(qkv, mask, lengths, B, S, NH):
    """attention_fp64 with the roundings of gpu_util.attention_rounded: the masked kernels round where the others do."""
    return _attention_eval(qkv, valid_keys(mask, lengths, S), B, S, NH, True)


def probs_fp64(qkv, mask, lengths, B, S, NH):
    """The attention probabilities [B, NH, S, S] in float64; masked keys' columns are exact zeros."""
    H = NH * 64
    x = qkv.double()
    heads = lambda t: t.reshape(B, S, NH, 64).permute(0, 2, 1, 3)
    s = (heads(x[:, :H]) @ heads(x[:, H:2 * H]).transpose(2, 3)) * ATTN_SCALE
    return torch.softmax(s.masked_fill(~valid_keys(mask, lengths, S)[:, None, None, :], float("-inf")), dim=-1)
