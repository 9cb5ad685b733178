"""Reference for the embedding inputs (token_type_ids / position_ids / inputs_embeds), on the CPU: the untouched
oracle/albert_np.py driven through a synthetic word table. The oracle embeds word[id] + type[0] + pos[s]; with one word row
per token, ids' = 1 + arange(B*S), and
    word'[1 + t] = base[t] + type[tt[t]] - type[0] + pos[pid[t]] - pos[s(t)]        (base = word[ids] or inputs_embeds)
its encoder_forward computes LN_E(base + type[tt] + pos[pid]) and everything above it, and the gradient encoder_backward
returns for word'[1:] is the gradient of the pre-LayerNorm sum per token. The three tables' gradients follow by np.add.at,
word row 0 (nn.Embedding's padding row) zeroed. tests/test_embed_inputs_host.py holds the construction to transformers."""
import numpy as np

from oracle import albert_np as onp

WORD = "encoder.embeddings.word_embeddings.weight"
POS = "encoder.embeddings.position_embeddings.weight"
TYPE = "encoder.embeddings.token_type_embeddings.weight"


def reference(ocfg, sd, lengths, dh, ids=None, token_type_ids=None, position_ids=None, inputs_embeds=None, dtype=np.float64):
    """(hidden [B,S,H], G, d_sum [B,S,E]): last_hidden_state, the gradients by name under `encoder.` for the upstream
    gradient dh (zeros at pad positions) — with inputs_embeds the word table's is zero — and the gradient of the
    pre-LayerNorm embedding sum per token. lengths None: no padding."""
    assert (ids is None) != (inputs_embeds is None)
    word, pos, typ = (np.asarray(sd[k], dtype) for k in (WORD, POS, TYPE))
    B, S = (np.asarray(ids).shape if ids is not None else np.asarray(inputs_embeds).shape[:2])
    T, E = B * S, word.shape[1]
    s_of_t = np.tile(np.arange(S), B)
    tt = np.zeros(T, np.int64) if token_type_ids is None else np.asarray(token_type_ids, np.int64).reshape(T)
    pid = s_of_t if position_ids is None else np.broadcast_to(np.asarray(position_ids, np.int64), (B, S)).reshape(T)
    base = word[np.asarray(ids).reshape(T)] if ids is not None else np.asarray(inputs_embeds, dtype).reshape(T, E)
    sd2 = dict(sd)
    sd2[WORD] = np.concatenate([np.zeros((1, E), dtype), base + typ[tt] - typ[0] + pos[pid] - pos[s_of_t]])
    am = None if lengths is None else onp.attention_mask_from_lengths(np.asarray(lengths))
    hidden, caches = onp.encoder_forward(ocfg, sd2, 1 + np.arange(T).reshape(B, S), am, dtype)
    G = dict(onp.encoder_backward(ocfg, sd2, caches, np.asarray(dh, dtype), dtype))
    d_sum = G[WORD][1:]
    dword, dpos, dtyp = np.zeros_like(word), np.zeros_like(pos), np.zeros_like(typ)
    if ids is not None:
        np.add.at(dword, np.asarray(ids).reshape(T), d_sum)
        dword[0] = 0
    np.add.at(dpos, pid, d_sum)
    np.add.at(dtyp, tt, d_sum)
    G[WORD], G[POS], G[TYPE] = dword, dpos, dtyp
    return hidden, G, d_sum.reshape(B, S, E)


def inputs(B, S, lengths, n_types, n_pos, E, seed):
    """The test inputs: random token types in [0, n_types), random positions in [0, n_pos), N(0,1) inputs_embeds."""
    rs = np.random.RandomState(seed)
    return (rs.randint(0, n_types, size=(B, S)).astype(np.int64), rs.randint(0, n_pos, size=(B, S)).astype(np.int64),
            rs.randn(B, S, E).astype(np.float32))
