"""float64 restatement of the pooler backward (include/plbert.h: plb_encode_bwd_pooled) and its error model. numpy only.

  pooled[b,:] = tanh(W · h0[b,:] + bias)          h0 = position 0 of the last hidden state (the fp32 image of bf16 rows)
  dpre   = d_pooled * (1 - y*y)                   y = pooled
  dW     = sum_b dpre[b,:]^T h0[b,:]
  db     = sum_b dpre[b,:]
  dh0[b] = dpre[b,:] · W

The error model, u = 2^-24 (fp32 round to nearest), no fitted constant:
  * a fixed-order fp32 sum of n products (with or without fused multiply-add): |error| <= (n + 2) u sum|a_i b_i|. The textbook
    bound is gamma_n = n u / (1 - n u); the two extra units cover the second-order terms for n <= 2^20 and the fact that the
    sum of magnitudes is taken over the float64 operands.
  * dpre, when y is taken from the bits plb_pooler returned: y*y, 1 - y*y and the product are one rounding each, at most
    (1 + 1 + 1) u |d_pooled| since |1 - y*y| <= 1 and y*y <= 1; 4 u |d_pooled| covers the second-order terms. This is what
    holds the backward to the forward's arithmetic: the bound leaves room for a y that differs from plb_pooler's by a unit
    or two in the last place (2 |y| times that), not for a y from other operands or a tanh of another accuracy class.
  * dW, db, dh0: their own sum bound plus the dpre bound propagated through the sum (each term's dpre error times the
    magnitude of the other operand).
"""
import numpy as np

U = 2.0 ** -24


def forward(h0, W, bias):
    h0, W, bias = (np.asarray(x, dtype=np.float64) for x in (h0, W, bias))
    return np.tanh(h0 @ W.T + bias)


def backward(h0, W, bias, d_pooled, y=None):
    """(dpre [B,H], dW [H,H], db [H], dh0 [B,H]) in float64; ``y``: the forward's output to differentiate at (default: the
    float64 forward)."""
    h0, W, d_pooled = (np.asarray(x, dtype=np.float64) for x in (h0, W, d_pooled))
    y = forward(h0, W, bias) if y is None else np.asarray(y, dtype=np.float64)
    dpre = d_pooled * (1.0 - y * y)
    return dpre, dpre.T @ h0, dpre.sum(axis=0), dpre @ W


def bounds(h0, W, d_pooled, y):
    """Elementwise bounds (e_dpre, e_dW, e_db, e_dh0) on |fp32 result - backward(..., y=y)| for fixed-order fp32 sums."""
    h0, W, d_pooled, y = (np.asarray(x, dtype=np.float64) for x in (h0, W, d_pooled, y))
    B, H = h0.shape
    dpre = np.abs(d_pooled * (1.0 - y * y))
    e_dpre = 4 * U * np.abs(d_pooled)
    e_dW = (B + 2) * U * (dpre.T @ np.abs(h0)) + e_dpre.T @ np.abs(h0)
    e_db = (B + 2) * U * dpre.sum(axis=0) + e_dpre.sum(axis=0)
    e_dh0 = (H + 2) * U * (dpre @ np.abs(W)) + e_dpre @ np.abs(W)
    return e_dpre, e_dW, e_db, e_dh0


def bf16_round(x):
    """float32 values rounded to nearest-even bf16, returned as float32 (the kernels' pack_bf2)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def fp32_emulation(h0, W, bias, d_pooled):
    """The sums in float32 numpy, one rounding per operation, each in ONE fixed order (b ascending, o ascending; the kernels cut
    the o sum in four and the forward dot by lanes: the bound is one for any fixed order, which is the subject here). Returns
    (y, dpre, dW, db, dh0), all float32."""
    f = np.float32
    h0, W, bias, d_pooled = (np.asarray(x, dtype=f) for x in (h0, W, bias, d_pooled))
    B, H = h0.shape
    pre = np.zeros((B, H), dtype=f)
    for k in range(H):
        pre = (pre + h0[:, k:k + 1] * W[:, k][None, :]).astype(f)
    y = np.tanh((pre + bias).astype(f)).astype(f)
    dpre = (d_pooled * (f(1) - (y * y).astype(f)).astype(f)).astype(f)
    dW, db = np.zeros((H, H), dtype=f), np.zeros(H, dtype=f)
    for b in range(B):
        dW = (dW + (dpre[b][:, None] * h0[b][None, :]).astype(f)).astype(f)
        db = (db + dpre[b]).astype(f)
    dh0 = np.zeros((B, H), dtype=f)
    for o in range(H):
        dh0 = (dh0 + (dpre[:, o:o + 1] * W[o][None, :]).astype(f)).astype(f)
    return y, dpre, dW, db, dh0
