"""numpy restatements of the masking kernels of csrc/mask.hip, written from their header comments: mask_words_kernel (the
Philox fast mode), apply_mask_kernel (host-drawn decisions) and the CSR compaction both share. Everything is integer work
or float32 comparisons of 24-bit uniforms, so the kernels are held to these bit for bit (tests/test_gpu_mask_kernels.py);
tests/test_mask_ref_host.py holds this file to the published Philox4x32-10 vectors and to the masking distribution."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the two multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key increments
MASK32 = 0xFFFFFFFF
MASK_ID, SEP_ID = 185, 186
DEFAULT_PROBS = (0.15, 0.8, 0.1)         # word_pred_prob, phoneme_mask_prob, replace_prob


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit values, key: two. Ten rounds of {hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0} with
    the key bumped after each; all arithmetic in uint64 masked to 32 bits. Returns four uint64 arrays of 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK32) for c in counter)
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    sh, lo32 = np.uint64(32), np.uint64(MASK32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2      # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & lo32, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & lo32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def u01(x):
    """float32(x >> 8) x 2^-24: 24 bits in [0, 1), exact in float32."""
    return (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def mask_words(labels, lengths, seed, step, probs=DEFAULT_PROBS, mask_id=MASK_ID, sep_id=SEP_ID):
    """labels int64 [B,S], lengths (B ints, or None = S). Per word (maximal run of non-separators inside the length), from
    the counter (word, b, step, 0) under the key (seed low, seed high): u1 < word_pred_prob selects it; then u2 <
    mask_prob -> every phoneme becomes mask_id; u2 < float32(mask_prob + replace_prob) -> phoneme i becomes
    pool[min(int(float32(u x float32(npool))), npool - 1)], u from the counter (i, b, step, 1), pool = the sample's phonemes
    in position order. `word` is the number of separators before the position. Returns (masked [B,S] int64, index lists):
    masked equals labels wherever no word was changed (past the length too); a list is ascending."""
    labels = np.asarray(labels, dtype=np.int64)
    B, S = labels.shape
    f = np.float32
    wp, mp, rp = f(probs[0]), f(probs[1]), f(probs[2])
    mr = f(mp + rp)
    key = (int(seed) & MASK32, (int(seed) >> 32) & MASK32)
    step = int(step) & MASK32
    masked = labels.copy()
    lists = []
    pos = np.arange(S)
    for b in range(B):
        n = S if lengths is None else min(max(int(lengths[b]), 0), S)
        inside = pos < n
        sep = inside & (labels[b] == sep_id)
        ph = inside & ~sep
        word = np.cumsum(sep) - sep                       # separators before the position
        pool = labels[b][ph]
        npool = int(pool.size)
        if npool == 0:
            lists.append(np.zeros(0, np.int32))
            continue
        r = philox4x32_10((word, b, step, 0), key)
        u1, u2 = u01(r[0]), u01(r[1])
        sel = ph & (u1 < wp)
        to_mask = sel & (u2 < mp)
        to_repl = sel & ~(u2 < mp) & (u2 < mr)
        c = philox4x32_10((pos, b, step, 1), key)
        pick = np.minimum((u01(c[0]) * f(npool)).astype(f).astype(np.int64), npool - 1)
        masked[b][to_mask] = mask_id
        masked[b][to_repl] = pool[pick[to_repl]]
        lists.append(np.flatnonzero(to_mask | to_repl).astype(np.int32))
    return masked, lists


def csr(lists):
    """(counts [B], offsets [B+1], flat) int32: the exclusive scan and the concatenation of the per-sample lists."""
    counts = np.array([len(x) for x in lists], dtype=np.int32)
    offsets = np.zeros(len(lists) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(counts)
    flat = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists]) if lists else np.zeros(0, np.int32)
    return counts, offsets, flat.astype(np.int32)


def words_of(row, n, sep_id=SEP_ID):
    """[(begin, end)] of the words of one sample inside its length."""
    out, start = [], None
    for i in range(n):
        if row[i] == sep_id:
            if start is not None:
                out.append((start, i))
                start = None
        elif start is None:
            start = i
    if start is not None:
        out.append((start, n))
    return out


def apply_mask(d, S, mask_id=MASK_ID, sep_token=0):
    """apply_mask_kernel on decision arrays in the layout of plbert_amd.data.collate_decisions (ids, repl, sample_off,
    word_off, word_begin, word_len, action, crop_start, word_token or None). Per sample: len = clip(n - crop_start, 0, S).
    Copy pass: labels = masked = ids[base + crop_start + i] for i < len, else 0; tokens = sep_token / 0. Word pass: every
    position word_begin + q - crop_start of a word that falls in [0, len): action 1 -> mask_id, 2 -> repl[base + word_begin
    + q] (the UNCROPPED position), tokens -> the word's token (action 0 too); actions 1 and 2 index the position. Returns
    dict(labels, masked, tokens or None, lengths, lists)."""
    B = len(d["crop_start"])
    with_tok = d.get("word_token") is not None
    labels = np.zeros((B, S), np.int64)
    masked = np.zeros((B, S), np.int64)
    tokens = np.zeros((B, S), np.int64) if with_tok else None
    lengths, lists = np.zeros(B, np.int32), []
    for b in range(B):
        base, n = int(d["sample_off"][b]), int(d["sample_off"][b + 1] - d["sample_off"][b])
        start = int(d["crop_start"][b])
        ln = min(max(n - start, 0), S)
        lengths[b] = ln
        labels[b, :ln] = masked[b, :ln] = d["ids"][base + start: base + start + ln]
        if with_tok:
            tokens[b, :ln] = sep_token
        flag = np.zeros(S, bool)
        for k in range(int(d["word_off"][b]), int(d["word_off"][b + 1])):
            wb, wl, act = int(d["word_begin"][k]), int(d["word_len"][k]), int(d["action"][k])
            for q in range(wl):
                i = wb + q - start
                if i < 0 or i >= ln:
                    continue
                if act == 1:
                    masked[b, i] = mask_id
                elif act == 2:
                    masked[b, i] = d["repl"][base + wb + q]
                if act != 0:
                    flag[i] = True
                if with_tok:
                    tokens[b, i] = d["word_token"][k]
        lists.append(np.flatnonzero(flag).astype(np.int32))
    return dict(labels=labels, masked=masked, tokens=tokens, lengths=lengths, lists=lists)


def random_labels(B, S, seed):
    """The label generator of tests/test_gpu_device_mask.py: words of 1-7 phonemes (ids 1..184) parted by separators; two
    rows in three run the whole S, the third ends somewhere in the upper half."""
    rs = np.random.RandomState(seed)
    lab = np.zeros((B, S), np.int64)
    lengths = []
    for b in range(B):
        L = S if b % 3 else int(rs.randint(S // 2, S + 1))
        pos = 0
        while pos < L:
            n = int(rs.randint(1, 8))
            end = min(pos + n, L)
            lab[b, pos:end] = rs.randint(1, 185, size=end - pos)
            if end < L:
                lab[b, end] = SEP_ID
            pos = end + 1
        lengths.append(L)
    return lab, lengths
