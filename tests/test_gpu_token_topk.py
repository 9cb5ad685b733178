"""The token top-k kernels at kernel level (-m gpu; csrc/token_topk.hip), launched through plb_launch_token_topk on synthetic
operands and held to tests/token_report_ref.py (which tests/test_token_report_host.py holds to torch):
 * exact case (integer operands, every partial sum an exact fp32 number): the logits output equals the float64 product bit for
   bit, ids / target_pos / totals equal the instrument — integer logits tie in large numbers, so this is the test of the
   (value, index) order across lanes, waves, tiles and strips;
 * real-valued case (one row with a NaN in X, a bias spike in the last column tile that makes the running maximum jump there):
   ids equal the instrument applied to the kernel's OWN logits, the logits are within the GEMM family's bound
   (K + 3) 2^-23 (sum |a||b| + |bias|) of float64, lse and the log-probabilities within the bound below of float64;
 * three runs bit-identical; ids and target_pos the same for every strip count, lse within the bound;
 * rows lists (shuffled, repeats, -1 entries), W rows behind NT full of NaN / 1e4, strides larger than K with junk in the gap,
   sentinel rows behind every output; plb_launch_token_topk_prepare against the instrument; the refusals.

Bound on lse and a log-probability (token_report_ref.logprob_bound): 1e-6 (|lse| + |z| + 1) + 1e-6 |value| — the tolerance
model of test_gpu_masked_report_rows.py for an fp32 evaluation of max + log(sum) - z with the hardware exp and log — plus
depth x 2^-24 for the sum of NT positive terms, depth = token_report_ref.sum_depth: per lane 17 roundings per column tile of
its strip (16 terms and one rescale), 14 for the 8 lanes of a row added in order, 7 for the butterfly over the strips.
Worst observed fraction of the bound over the real-valued shapes, first run on an MI355X (pytest -s prints it per case):
0.007 / 0.029 / 0.032 / 0.035 / 0.019 / 0.042 / 0.037 / 0.036 in the order of SHAPES — the 1e-6 |lse| term dominates the bound
(the spike puts lse near 25), the summation term is never approached."""
import numpy as np
import pytest
import torch

from gpu_util import EXACT_LIMIT, exact_bound, int_bias, int_operands, stream
import token_report_ref as ref
from plbert_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 3
I_SENT, F_SENT = -77, 7.0
# (n, NT, K): 1 / 127 / 129 / 300 rows (one lane group, a short tile, a second tile, three tiles); NT below one MFMA tile,
# below / at / just past one column tile, 8 and 40 column tiles (strips of several tiles); one, two and twelve K tiles
SHAPES = [(1, 5, 64), (127, 96, 128), (129, 128, 64), (300, 129, 128), (1, 1000, 128), (129, 1000, 768), (300, 5000, 128),
          (127, 5000, 768)]
STRIPS = (1, 3, 16, 0)
TOPKS = (0, 1, 5, 8)


def _rup(x, m):
    return (x + m - 1) // m * m


def _buffers(Xv, Wv, NT, K, seed):
    """X [nx][K + 8] and W [rup(NT, 128)][K + 16] bf16 on the device: junk in the gap behind K, NaN and 1e4 rows behind NT."""
    g = torch.Generator().manual_seed(seed)
    nx = Xv.shape[0]
    X = torch.full((nx, K + 8), 777.0, dtype=torch.bfloat16)
    X[:, :K] = Xv
    W = torch.full((_rup(NT, 128), K + 16), 777.0, dtype=torch.bfloat16)
    W[:NT, :K] = Wv
    tail = torch.where(torch.rand((W.shape[0] - NT, K), generator=g) < 0.5, float("nan"), 1e4).to(torch.bfloat16)
    W[NT:, :K] = tail
    return X.to(DEV), W.to(DEV)


def _row_list(n, nx, seed):
    """Shuffled, with repeats and -1 entries (none where n == 1: that row is then the case's only one)."""
    g = np.random.default_rng(seed)
    rows = g.integers(0, nx, size=n).astype(np.int32)
    if n > 1:
        rows[g.random(n) < 0.1] = -1
        rows[1] = -1
        rows[0] = rows[n - 1] = nx - 1
    return rows


def _launch(X, W, bias, rows, tgt, n, NT, K, topk, strips, logits=True, totals=True):
    L = _lib.lib()
    scratch = torch.empty(int(L.plb_token_topk_scratch_bytes(n)) // 4 + GUARD, dtype=torch.int32, device=DEV)
    scratch.fill_(I_SENT)
    k1 = max(topk, 1)
    out = {"ids": torch.full((n + GUARD, k1), I_SENT, dtype=torch.int32, device=DEV),
           "lp": torch.full((n + GUARD, k1), F_SENT, device=DEV),
           "lse": torch.full((n + GUARD,), F_SENT, device=DEV),
           "tlp": torch.full((n + GUARD,), F_SENT, device=DEV),
           "pos": torch.full((n + GUARD,), I_SENT, dtype=torch.int32, device=DEV),
           "logits": torch.full((n + GUARD, NT), F_SENT, device=DEV),
           "totals": torch.full((3 + GUARD,), I_SENT, dtype=torch.int32, device=DEV)}
    p = lambda t: None if t is None else t.data_ptr()
    has_t = tgt is not None
    rc = L.plb_launch_token_topk(X.data_ptr(), X.shape[1], p(rows), n, W.data_ptr(), W.shape[1], bias.data_ptr(), NT, K, topk,
                                 strips, scratch.data_ptr(), p(tgt), out["ids"].data_ptr(), out["lp"].data_ptr(),
                                 out["lse"].data_ptr(), p(out["tlp"]) if has_t else None, p(out["pos"]) if has_t else None,
                                 p(out["logits"]) if logits else None, p(out["totals"]) if (totals and has_t) else None, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((scratch[-GUARD:] == I_SENT).all())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_guards(got, n, topk, has_t=True, logits=True):
    for k, sent in (("ids", I_SENT), ("lp", F_SENT), ("lse", F_SENT), ("tlp", F_SENT), ("pos", I_SENT), ("logits", F_SENT)):
        assert bool((got[k][n:] == sent).all()), k
    assert bool((got["totals"][3:] == I_SENT).all())
    if not topk:
        assert bool((got["ids"] == I_SENT).all()) and bool((got["lp"] == F_SENT).all())
    if not has_t:
        assert bool((got["tlp"] == F_SENT).all()) and bool((got["pos"] == I_SENT).all()) and bool((got["totals"] == I_SENT).all())
    if not logits:
        assert bool((got["logits"] == F_SENT).all())


def _check_discrete(got, want, n, topk):
    if topk:
        assert np.array_equal(got["ids"][:n, :topk], want.topk_ids), np.argwhere(got["ids"][:n, :topk] != want.topk_ids)[:5]
    assert np.array_equal(got["pos"][:n], want.target_pos)
    assert np.array_equal(got["totals"][:3], want.totals)


def _check_values(got, want, z64, n, NT, topk, nstrips):
    """lse / log-probabilities against float64 within logprob_bound; the NaN and -inf patterns exactly. Returns the worst
    observed fraction of the bound."""
    worst = 0.0
    ok = ~(want.nan | want.norow)
    lse = got["lse"][:n].astype(np.float64)
    assert np.isnan(lse[~ok]).all()
    b = ref.logprob_bound(want.lse[ok], 0.0, want.lse[ok], NT, nstrips)
    err = np.abs(lse[ok] - want.lse[ok])
    assert bool((err <= b).all()), float((err / b).max())
    worst = max(worst, float((err / b).max()) if ok.any() else 0.0)
    tlp = got["tlp"][:n].astype(np.float64)
    fin = np.isfinite(want.target_logprob)
    assert np.isnan(tlp[~fin]).all()
    if fin.any():
        b = ref.logprob_bound(want.lse[fin], want.target_logprob[fin] + want.lse[fin], want.target_logprob[fin], NT, nstrips)
        err = np.abs(tlp[fin] - want.target_logprob[fin])
        assert bool((err <= b).all()), float((err / b).max())
        worst = max(worst, float((err / b).max()))
    if topk:
        lp, wlp = got["lp"][:n, :topk].astype(np.float64), want.topk_logprob
        assert np.isnan(lp[want.nan]).all() and np.isneginf(lp[want.norow]).all()
        assert np.array_equal(np.isneginf(lp[ok]), np.isneginf(wlp[ok]))
        fin = np.isfinite(wlp) & ok[:, None]
        if fin.any():
            b = ref.logprob_bound(want.lse[:, None], wlp + want.lse[:, None], wlp, NT, nstrips)
            err = np.abs(np.where(fin, lp, 0.0) - np.where(fin, wlp, 0.0))
            assert bool((err[fin] <= b[fin]).all()), float((err[fin] / b[fin]).max())
            worst = max(worst, float((err[fin] / b[fin]).max()))
    return worst


def _gather64(Xv, rows, n):
    idx = np.arange(n) if rows is None else np.where(rows < 0, 0, rows)
    return Xv.double().numpy()[idx]


@pytest.mark.parametrize("listed", [False, True], ids=["identity", "rowlist"])
@pytest.mark.parametrize("n,NT,K", SHAPES)
def test_exact_case(n, NT, K, listed):
    nx = max(n, 40) if listed else n
    Xv = int_operands((nx, K), -4, 4, seed=n + NT)
    Wv = int_operands((NT, K), -4, 4, seed=n + NT + 1)
    bias = int_bias(NT, seed=K, hi=8)
    assert exact_bound(Xv, Wv, bias) < EXACT_LIMIT
    X, W = _buffers(Xv, Wv, NT, K, seed=NT)
    rows = _row_list(n, nx, seed=n) if listed else None
    z = _gather64(Xv, rows, n) @ Wv.double().numpy().T + bias.double().numpy()
    g = np.random.default_rng(NT + n)
    tgt = g.integers(0, NT, size=n).astype(np.int32)
    tgt[0] = int(np.argmax(z[0]))                                   # (np.argmax: the lowest index of the maximum) a hit
    d_rows = None if rows is None else torch.from_numpy(rows).to(DEV)
    d_tgt, d_bias = torch.from_numpy(tgt).to(DEV), bias.to(DEV)
    live = np.ones(n, bool) if rows is None else rows >= 0
    for topk, strips in [(k, 0) for k in TOPKS] + [(5, s) for s in STRIPS[:3]]:
        got = _launch(X, W, d_bias, d_rows, d_tgt, n, NT, K, topk, strips)
        want = ref.report(z, tgt, topk, rows)
        _check_guards(got, n, topk)
        assert np.array_equal(got["logits"][:n][live].astype(np.float64), z[live]), (topk, strips)
        assert bool((got["logits"][:n][~live] == 0).all())
        _check_discrete(got, want, n, topk)
        _check_values(got, want, z, n, NT, topk, ref.strips(n, NT, strips))
    assert want.totals[0] == int(live.sum())
    # without targets, without the logits copy: only what is asked for is written
    got = _launch(X, W, d_bias, d_rows, None, n, NT, K, 5, 0, logits=False)
    _check_guards(got, n, 5, has_t=False, logits=False)
    assert np.array_equal(got["ids"][:n, :5], ref.report(z, None, 5, rows).topk_ids)


@pytest.mark.parametrize("n,NT,K", SHAPES)
def test_real_valued_case(n, NT, K):
    g = torch.Generator().manual_seed(7 * n + NT + K)
    nx = max(n, 40)
    Xv = torch.randn((nx, K), generator=g).to(torch.bfloat16)
    Wv = (torch.randn((NT, K), generator=g) * (2.0 / K ** 0.5)).to(torch.bfloat16)
    bias = torch.randn((NT,), generator=g) * 0.5
    spike = NT - 2 if NT > 2 else 0
    bias[spike] += 25.0                                             # the running maximum jumps in the LAST column tile
    rows = _row_list(n, nx, seed=n + 1)
    if n > 2:                                                       # one position reads a row of X that holds a NaN
        rows[n // 2] = 3
        Xv[3, K // 2] = float("nan")
    X, W = _buffers(Xv, Wv, NT, K, seed=NT + 1)
    A = _gather64(Xv, rows, n)
    z64 = A @ Wv.double().numpy().T + bias.double().numpy()
    mag = np.abs(np.nan_to_num(A)) @ np.abs(Wv.double().numpy()).T + np.abs(bias.double().numpy())
    tgt = np.random.default_rng(n).integers(0, NT, size=n).astype(np.int32)
    tgt[::3] = spike
    d_rows, d_tgt, d_bias = torch.from_numpy(rows).to(DEV), torch.from_numpy(tgt).to(DEV), bias.to(DEV)
    live = rows >= 0
    worst, per_strips = 0.0, {}
    for topk, strips in [(k, 0) for k in TOPKS] + [(5, s) for s in STRIPS[:3]]:
        runs = [_launch(X, W, d_bias, d_rows, d_tgt, n, NT, K, topk, strips) for _ in range(3 if topk == 5 else 1)]
        for r in runs[1:]:                                          # bitwise reproducible
            assert all(np.array_equal(r[k].view(np.uint32), runs[0][k].view(np.uint32)) for k in r), strips
        got = runs[0]
        _check_guards(got, n, topk)
        zk = got["logits"][:n].astype(np.float64)                   # the kernel's own logits
        fin = live[:, None] & np.isfinite(z64)
        err = np.abs(np.where(fin, zk - z64, 0.0))
        assert bool((err <= (K + 3) * 2.0 ** -23 * mag + 1e-30).all()), float((err / ((K + 3) * 2.0 ** -23 * mag + 1e-30)).max())
        assert np.array_equal(np.isnan(zk[live]), np.isnan(z64[live])) and bool((zk[~live] == 0).all())
        want = ref.report(zk, tgt, topk, rows)
        _check_discrete(got, want, n, topk)
        worst = max(worst, _check_values(got, want, zk, n, NT, topk, ref.strips(n, NT, strips)))
        if topk == 5:
            per_strips[strips] = got
        if topk and live[0] and not want.nan[0]:
            assert got["ids"][0, 0] == spike and abs(got["lp"][0, 0]) < 1e-3     # the spike leads, with probability ~1
    print(f"\ntoken_topk n={n} NT={NT} K={K}: worst fraction of the lse / log-probability bound {worst:.3f}")
    base = per_strips[0]
    for s, got in per_strips.items():                               # the order is defined on (value, index): no strip count changes it
        assert np.array_equal(got["ids"], base["ids"]) and np.array_equal(got["pos"], base["pos"]), s
        assert np.array_equal(got["totals"], base["totals"]) and np.array_equal(got["logits"].view(np.uint32), base["logits"].view(np.uint32))
        ok = np.isfinite(base["lse"][:n])
        b = ref.logprob_bound(base["lse"][:n][ok], 0.0, base["lse"][:n][ok], NT, 1)
        assert bool((np.abs(got["lse"][:n][ok].astype(np.float64) - base["lse"][:n][ok]) <= 2 * b).all()), s


def test_prepare_against_the_instrument():
    L = _lib.lib()
    B, S = 3, 40
    lengths = np.array([40, 33, 7], np.int32)
    g = np.random.default_rng(3)
    tok = g.integers(0, 96, size=(B, S)).astype(np.int64)
    counts = [5, 0, 4]
    flat = np.concatenate([g.choice(40, 5, replace=False), g.choice(7, 4, replace=False)]).astype(np.int32)
    flat[2] = 39
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    row_start = np.array([0, 128, 256, 384], np.int32)
    dv = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    d_tok = dv(tok)
    for offs, fl, n in ((offsets, flat, len(flat)), (None, None, B * S)):
        for lens in (lengths, None):
            for rs in (None, row_start):
                for tk in (tok, None):
                    rows = torch.full((n + GUARD,), I_SENT, dtype=torch.int32, device=DEV)
                    tgt = torch.full((n + GUARD,), I_SENT, dtype=torch.int32, device=DEV)
                    d = [dv(offs), dv(fl), dv(lens), dv(rs)]
                    p = lambda t: None if t is None else t.data_ptr()
                    assert L.plb_launch_token_topk_prepare(p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(d_tok) if tk is not None else None,
                                                           n, B, S, rows.data_ptr(), tgt.data_ptr(), stream()) == 0
                    torch.cuda.synchronize()
                    wr, wt = ref.prepare(offs, fl, lens, rs, tk, n, B, S)
                    assert np.array_equal(rows.cpu().numpy()[:n], wr) and np.array_equal(tgt.cpu().numpy()[:n], wt)
                    assert bool((rows[n:] == I_SENT).all()) and bool((tgt[n:] == I_SENT).all())
    # the full form needs n == B*S
    buf = torch.zeros(256, dtype=torch.int32, device=DEV)
    assert L.plb_launch_token_topk_prepare(None, None, None, None, None, B * S - 1, B, S, buf.data_ptr(), buf.data_ptr(), stream()) != 0


def test_refuses_what_it_cannot_run():
    L = _lib.lib()
    buf = torch.zeros(1 << 16, device=DEV)
    p = buf.data_ptr()

    def rc(n=4, NT=96, K=64, topk=5, strips=0, ldx=64, ldw=64, tgt=p, tlp=p, totals=p):
        return L.plb_launch_token_topk(p, ldx, None, n, p, ldw, p, NT, K, topk, strips, p, tgt, p, p, p, tlp, p, p, totals, stream())
    assert rc(topk=9) != 0 and rc(topk=-1) != 0 and rc(K=96) != 0 and rc(K=0) != 0 and rc(strips=17) != 0 and rc(strips=-1) != 0
    assert rc(ldx=32) != 0 and rc(ldw=60) != 0 and rc(ldx=68) != 0 and rc(NT=0) != 0 and rc(n=-1) != 0
    assert rc(tgt=None) != 0 and rc(tgt=None, tlp=None) != 0               # target outputs / totals need targets
    torch.cuda.synchronize()
    assert bool((buf == 0).all())                                          # nothing was launched
    tot = torch.full((3 + GUARD,), I_SENT, dtype=torch.int32, device=DEV)
    assert rc(n=0, totals=tot.data_ptr()) == 0                             # no rows: zeros in totals, nothing else
    torch.cuda.synchronize()
    assert tot.cpu().tolist() == [0, 0, 0] + [I_SENT] * GUARD and bool((buf == 0).all())
