"""The instrument of the masked-report tests: a numpy restatement of what plb_launch_masked_report_rows / _samples and
plb_launch_token_top1 define (csrc/plbert_kernels.h), independent of torch and of the kernels. tests/test_masked_report_host.py
holds it against torch on the CPU; the GPU tests hold the kernels and plb_masked_report against it.

Order of the classes of a row: (logit descending, class index ascending) — among equal logits the lowest index wins."""
import numpy as np

U32 = 2.0 ** -24   # unit roundoff of fp32


class Rows:
    def __init__(self, pred, rank, nll, lse, topk_ids, topk_logprob, nan):
        self.pred, self.rank, self.nll, self.lse = pred, rank, nll, lse
        self.topk_ids, self.topk_logprob, self.nan = topk_ids, topk_logprob, nan


def order(z):
    """Class indices of one row in report order (a stable sort of -z keeps ascending indices among equals)."""
    return np.argsort(-np.asarray(z, np.float64), kind="stable")


def rows(z, tgt, topk):
    """z [n, V] (any float type, evaluated in float64), tgt [n] -> Rows with pred / rank int32 [n], nll / lse float64 [n],
    topk_ids int32 [n, topk], topk_logprob float64 [n, topk]. Entries of the list past V: id -1, logprob -inf. A row with a
    NaN logit: pred -1, rank V, nll NaN, ids -1, logprobs NaN."""
    z = np.asarray(z, np.float64)
    tgt = np.asarray(tgt, np.int64)
    n, V = z.shape
    pred = np.full(n, -1, np.int32)
    rank = np.full(n, V, np.int32)
    nll = np.full(n, np.nan)
    lse = np.full(n, np.nan)
    ids = np.full((n, topk), -1, np.int32)
    lp = np.full((n, topk), -np.inf)
    nan = np.isnan(z).any(1)
    for j in range(n):
        if nan[j]:
            lp[j] = np.nan
            continue
        zj, t = z[j], int(tgt[j])
        m = zj.max()
        lse[j] = m + np.log(np.exp(zj - m).sum())
        nll[j] = lse[j] - zj[t]
        rank[j] = int((zj > zj[t]).sum() + (zj[:t] == zj[t]).sum())
        o = order(zj)
        pred[j] = o[0]
        k = min(topk, V)
        ids[j, :k] = o[:k]
        lp[j, :k] = zj[o[:k]] - lse[j]
    return Rows(pred, rank, nll, lse, ids, lp, nan)


class Samples:
    def __init__(self, loss, top1, topk, totals):
        self.loss, self.top1, self.topk, self.totals = loss, top1, topk, totals


def count_threshold(topk, V):
    """What plb_masked_report hands the sample launch as its top-k threshold: min(topk, V), so that the rank V of a NaN
    row never counts, also where the list is longer than the vocabulary."""
    return min(int(topk), int(V))


def samples(offsets, rank, nll, topk):
    """CSR offsets [B+1], rank [n], nll [n] -> per-sample mean nll (float64; 0 for a sample without rows), counts of
    rank == 0 and rank < topk (int32 [B]) and totals int32 [4] = {rows, top-1 correct, top-k correct, samples with rows}.
    topk is the counting threshold (count_threshold)."""
    offsets = np.asarray(offsets, np.int64)
    rank = np.asarray(rank, np.int64)
    nll = np.asarray(nll, np.float64)
    B = len(offsets) - 1
    loss = np.zeros(B)
    top1 = np.zeros(B, np.int32)
    tk = np.zeros(B, np.int32)
    for b in range(B):
        a, e = int(offsets[b]), int(offsets[b + 1])
        if e > a:
            loss[b] = nll[a:e].sum() / (e - a)
        top1[b] = int((rank[a:e] == 0).sum())
        tk[b] = int((rank[a:e] < topk).sum())
    n = int(offsets[B])
    totals = np.array([n, int((rank[:n] == 0).sum()), int((rank[:n] < topk).sum()), int((np.diff(offsets) > 0).sum())], np.int32)
    return Samples(loss, top1, tk, totals)


def sample_loss_bound(offsets, nll):
    """What fp32 may lose on sample_loss[b]: the kernel adds a sample's n_b rows in chains of ceil(n_b / 256) terms per
    thread, 6 butterfly steps and 3 additions over the waves (the depth test_gpu_rowops.test_sum_rows states for the same
    order), then divides once: (depth + 1) roundings of at most the sum of magnitudes, over n_b."""
    offsets = np.asarray(offsets, np.int64)
    nll = np.abs(np.asarray(nll, np.float64))
    out = np.zeros(len(offsets) - 1)
    for b in range(len(out)):
        a, e = int(offsets[b]), int(offsets[b + 1])
        if e > a:
            out[b] = (-(-(e - a) // 256) + 9 + 1) * U32 * nll[a:e].sum() / (e - a)
    return out


def token_top1(pmax, tlogit, w):
    """pmax [rows, ntiles], tlogit [rows], w [rows] -> int32 [2] = {rows with w != 0, those whose target logit EQUALS the
    maximum of the row's per-tile maxima}: tie-inclusive."""
    pmax, tlogit, w = np.asarray(pmax), np.asarray(tlogit), np.asarray(w)
    valid = w != 0
    return np.array([int(valid.sum()), int((valid & (tlogit == pmax.max(1))).sum())], np.int32)
