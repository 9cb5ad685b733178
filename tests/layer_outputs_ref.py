"""Float64 references of the per-application outputs (include/plbert.h: PlbLayerOutputs, plb_encode_bwd_layers), for the
host tests (tests/test_layer_outputs_host.py) and the -m gpu tests of the two kernels and of the engine.

 - attn_probs_ref: what plb_launch_attn_probs stands for — softmax over the valid keys of scale * q·k, zeros in pad key
   columns AND pad query rows (the library's deviation from HuggingFace, as plb_encode's).
 - add_row_grad_ref: bf16(float(res) + g) on the rows of valid positions, res elsewhere.
 - layer_gradient_sum: the parameter gradient of sum_l <G_l, hidden_states[l]> from the UNCHANGED oracle. hidden_states[l]
   is the output of a model with l applications, and the first l entries of caches["layers"] are exactly that model's
   caches (the layer is shared and application l reads only what came before), so
       d/dP sum_l <G_l, hidden_states[l]> = sum_l encoder_backward(cfg, P, caches with layers[:l], G_l)
   (encoder_backward walks caches["layers"] and nothing else of the depth; layers[:0] leaves the map-in / embedding term).
   tests/test_layer_outputs_host.py proves it against central finite differences."""
import numpy as np
import torch

from oracle import albert_np as onp


def valid_mask(lengths, S):
    return np.arange(S)[None, :] < np.asarray(lengths)[:, None]


def attn_probs_ref(q, k, lengths, scale):
    """q, k [B,NH,S,d] (any float dtype: the values as the kernel reads them) -> float64 [B,NH,S,S]."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    B, NH, S, _ = q.shape
    out = np.zeros((B, NH, S, S), np.float64)
    for b in range(B):
        n = int(min(max(int(lengths[b]), 1), S))
        s = (q[b, :, :n] @ k[b, :, :n].transpose(0, 2, 1)) * scale
        s = s - s.max(-1, keepdims=True)
        p = np.exp(s)
        out[b, :, :n, :n] = p / p.sum(-1, keepdims=True)
    return out


def token_rows(lengths, S, row_start=None):
    """(positions, rows): for every valid (b, s), in (b, s) order, its flat position b*S + s in a [B,S,*] tensor and its row
    of the call's token axis (row_start: the plan's table; None: the padded layout, where the two are equal)."""
    pos, rows = [], []
    for b, n in enumerate(np.asarray(lengths)):
        n = int(min(max(int(n), 1), S))
        pos.append(np.arange(n) + b * S)
        rows.append(np.arange(n) + (b * S if row_start is None else int(row_start[b])))
    return torch.as_tensor(np.concatenate(pos)), torch.as_tensor(np.concatenate(rows))


def add_row_grad_ref(res, g, positions, rows):
    """res bf16 [Tp,H], g fp32 [B,S,H] (torch, CPU), positions / rows from token_rows -> bf16 [Tp,H]: torch's fp32 sum and
    round-to-nearest-even conversion on the rows of valid positions, res itself on every other row."""
    out = res.clone()
    out[rows] = (res[rows].float() + g.reshape(-1, g.shape[-1])[positions]).to(torch.bfloat16)
    return out


def hidden_states_of(hidden, caches):
    """[hidden_states[0], ..., hidden_states[L]] of an oracle forward: the input of every application, then the output."""
    return [c["x"] for c in caches["layers"]] + [hidden]


def layer_gradient_sum(ocfg, sd, caches, Gs, dtype=np.float64):
    """Gs: L + 1 arrays [B,S,H] or None (G_l = d loss / d hidden_states[l]) -> {name: gradient} over the encoder tensors."""
    total = {}
    for l, G in enumerate(Gs):
        if G is None:
            continue
        part = onp.encoder_backward(ocfg, sd, dict(caches, layers=caches["layers"][:l]), np.asarray(G, dtype), dtype)
        for k, v in part.items():
            total[k] = total[k] + v if k in total else v.copy()
    return total
