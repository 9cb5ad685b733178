"""The instrument of the token-report tests: a numpy restatement of what plb_launch_token_topk / plb_launch_token_topk_prepare
define (csrc/plbert_kernels.h) and plb_token_report hands out (include/plbert.h), on top of masked_report_ref.rows — the same
order of classes: (logit descending, class index ascending). Independent of torch and of the kernels;
tests/test_token_report_host.py holds it against torch on the CPU, the GPU tests hold the kernels and the entry point against it.

Beside masked_report_ref.rows' rules (entries of the list past the vocabulary: id -1, -inf; a row with a NaN logit: ids -1,
log-probabilities and lse NaN) a row list entry of -1 marks a position WITHOUT A ROW: ids -1, log-probabilities -inf, lse and
target_logprob NaN, target_pos -1, logits 0, never counted."""
import numpy as np

import masked_report_ref as mref

U32 = mref.U32


class Report:
    def __init__(self, topk_ids, topk_logprob, lse, target_logprob, target_pos, totals, nan, norow):
        self.topk_ids, self.topk_logprob, self.lse = topk_ids, topk_logprob, lse
        self.target_logprob, self.target_pos, self.totals = target_logprob, target_pos, totals
        self.nan, self.norow = nan, norow


def report(z, tgt, topk, rows=None):
    """z [n, NT] the logits of the n positions (any float type, evaluated in float64; the values at a position without a row
    are ignored), tgt [n] or None, rows [n] or None (only its sign is read: < 0 = no row) -> Report with topk_ids int32
    [n, topk], topk_logprob / lse / target_logprob float64, target_pos int32 [n] (the 0-based position of tgt in the list,
    -1 when it is not among the first topk — or the row has a NaN, or no row, or tgt lies outside [0, NT)), totals int32 [3] =
    {positions that have a row, target_pos == 0, target_pos >= 0}."""
    z = np.asarray(z, np.float64)
    n, NT = z.shape
    norow = np.zeros(n, bool) if rows is None else np.asarray(rows) < 0
    has_t = tgt is not None
    t = np.asarray(tgt, np.int64) if has_t else np.full(n, -1, np.int64)
    in_range = (t >= 0) & (t < NT)
    base = mref.rows(np.where(norow[:, None], 0.0, z), np.clip(t, 0, NT - 1), topk)
    ids, lp, lse = base.topk_ids.copy(), base.topk_logprob.copy(), base.lse.copy()
    nan = base.nan & ~norow
    ids[norow] = -1
    lp[norow] = -np.inf
    lse[norow] = np.nan
    tlp = np.full(n, np.nan)
    pos = np.full(n, -1, np.int32)
    for j in range(n):
        if norow[j] or nan[j] or not in_range[j]:
            continue
        tlp[j] = z[j, t[j]] - lse[j]
        hit = np.nonzero(ids[j] == t[j])[0]
        if len(hit):
            pos[j] = int(hit[0])
    totals = np.array([int((~norow).sum()), int((pos == 0).sum()), int((pos >= 0).sum())], np.int32)
    return Report(ids, lp, lse, tlp, pos, totals, nan, norow)


def prepare(offsets, flat, lengths, row_start, token_ids, n, B, S):
    """plb_launch_token_topk_prepare: (rows int32 [n], tgt int32 [n]). CSR form (offsets given) or every position of [B,S]."""
    rows = np.full(n, -1, np.int32)
    tgt = np.full(n, -1, np.int32)
    for j in range(n):
        if offsets is not None:
            b = int(np.searchsorted(np.asarray(offsets)[:B], j, side="right") - 1)
            s = int(flat[j])
        else:
            b, s = divmod(j, S)
        ln = S if lengths is None else min(max(int(lengths[b]), 1), S)
        if 0 <= s < ln:
            rows[j] = (b * S if row_start is None else int(row_start[b])) + s
            if token_ids is not None:
                tgt[j] = int(np.asarray(token_ids).reshape(B, S)[b, s])
    return rows, tgt


def strips(n, NT, forced=0, max_strips=16):
    """plb_token_topk_strips."""
    if n < 1 or NT < 1:
        return 0
    row_tiles, ntiles = -(-n // 128), -(-NT // 128)
    s = forced if forced else -(-512 // row_tiles)
    s = min(s, max_strips, ntiles)
    per = -(-ntiles // s)
    return -(-ntiles // per)


def sum_depth(NT, nstrips):
    """Longest chain of fp32 additions behind the sum of exponentials of one row (csrc/token_topk.hip): a lane adds the 16
    terms of each of its strip's column tiles to a running sum that it rescales once per tile (17 roundings per tile), the 8
    lanes that share a row are added in order (7, each behind a rescale: 14), the strips meet in a 6-step butterfly behind
    one rescale each (7)."""
    ntiles = -(-NT // 128)
    per = -(-ntiles // nstrips)
    return 17 * per + 14 + 7


def logprob_bound(lse, z, value, NT, nstrips):
    """What fp32 may lose on lse (value = lse, z = 0) or on a log-probability z - lse: the tolerance model of
    test_gpu_masked_report_rows.py — 1e-6 of |lse| + |z| + 1 and 1e-6 of the value, for the hardware exp / log and the few
    roundings of operands of those magnitudes — plus depth x 2^-24 for a sum of NT positive terms added in chains of that
    depth: a relative error of depth x u on the sum is an absolute one on its logarithm."""
    return 1e-6 * (np.abs(lse) + np.abs(z) + 1) + 1e-6 * np.abs(value) + sum_depth(NT, nstrips) * U32
