"""The fused token-head cross-entropy (plb_launch_gemm_nt_big act 3 -> plb_launch_token_ce_combine[_packed] -> act 4 -> the
bias column sums) without a GPU: the case table, a float64 reference, the kernels' algorithm restated in fp32, and the
per-element checker that tests/test_gpu_token_ce.py runs the kernels through and tests/test_token_ce_host.py proves on the
CPU. Plain torch; only launch() touches ctypes.

CASES. M = 256 rows (one row tile of the 256x256 form, two of the 128x256 form), K = 64, (N, ce_cols) from TABLE. Operands
are integers times UNIT = 2^-4, so every logit is an exact fp32 number whatever the summation order (premise(): the sum of
the terms' magnitudes stays below 2^24 units — asserted before every launch, a condition and not a tolerance). Column k of
W is a logit profile and a row of A picks profiles by its k-th entries:
    k 0..3   soft profiles, integers in [-8, 8] units (spread 1), 0 at the indicator columns
    k 4      the offset profile, 16.0 everywhere; the bias is -80 (+ jitter of +-4 units, 0 at the indicator columns), so a
             row with coefficient 5 sits near 0, with 10 near +80 and with 0 near -80 (through the bias alone)
    k 5..10  indicators: 16.0 at ONE column (positions(): tile 0 twice, the last real class, a tile that is a lane's second
             iteration of the merge, one that is its last, a lower-indexed tile of the same lane), 0 elsewhere
so `soft + 2 x indicator` is a sharp row (gap 32; 5 -> 80, 8 -> 128), two indicators an exact tie. Columns >= ce_cols carry
bias +1000: a padding column that were counted would dominate its row. Rows of weight 0 (pad positions, the rest of a
packed slot, rows >= B*S) hold +inf, -inf, NaN or 3e38 in A and the targets -1, ce_cols, N + 5 and 2^40. One further case
("gauss") has Gaussian operands with K = 192; it is not exact and carries dz = (K + 3) 2^-23 (sum |a||b| + |bias|) as the
bound on every logit's error.

ALLOWANCES (u = 2^-24; allowances() computes them from the float64 reference alone).
  e_exp(x) = (|x| log2(e) + 1) 2^-23 + |x| u     relative error of __expf(x) = v_exp_f32(x * log2 e): the fp32 product
             and the rounded constant move the exponent by |x| log2(e) 2^-23, the instruction is accurate to 1 ulp (the
             ISA's figure for V_EXP_F32, and for V_LOG_F32 below), and |x| u is the rounding of the difference x itself.
  psum     relative 256 u + e_exp(the tile's widest argument) [+ 2 dz]. The exponents along a value's way through the
             lane, four-lane and four-wave merges are all <= 0 and add up to (z - tile maximum), so their |x| terms
             telescope into one e_exp; 256 u covers the 22 additions, the 6 rescales' two roundings and their constants.
  lse      absolute d_lse = sum_tiles share_i (psum_i's relative + |pmax_i - M| (log2(e) 2^-23 + u))
                            + 10 (2^-23 + 2 u) + 10 u        the longest chain: 4 tiles per lane + 6 wave steps, per step
                                                             one exponential's constant, two products, one addition
                            + |ln l| 2^-22                   __logf: v_log_f32 to 1 ulp, times ln 2 in fp32
                            + u |lse| [+ max dz of the row]
  loss     w (d_lse + 2^-23 (|lse| + |z_t|)) [+ w dz_t]
  gradient one bf16 spacing of the reference element + w p (d_lse + dz + e_exp(z - lse)) + u w p (the product)
             + u w on the target column (the subtraction)
  colpart  |colpart[2t] + colpart[2t+1] - column sums of the STORED rows of row tile t| <= (TM/2 + 1) u sum |stored|,
             exactly 0 on columns >= ce_cols
  bias gradient (plb_launch_colsum over colpart): (TM/2 + 1 + rows of colpart + 11) u sum |stored| against the float64
             column sums of the stored gradient (the partial's chain, one row per partial, the launch's 8-way tree)
  underflow  an element whose reference magnitude is below w 2^-100 is checked absolutely, |got| <= w 2^-100; how many
             there are is counted from the reference (floor_count) and asserted against the designed number.
Exact by contract: pmax / tlogit (exact cases, valid rows), w, (-inf, 0) on a tile without a real class, zeros of lse / w /
loss on rows of weight 0, zeros of the gradient on rows of weight 0, rows >= B*S and columns >= ce_cols, the top-1 totals.
"""
import functools
from types import SimpleNamespace as NS

import torch

from gpu_util import spacing_bf16

U = 2.0 ** -24
LOG2E = 1.4426950408889634
FLOOR = 2.0 ** -100
UNIT = 2.0 ** -4
M = 256
TABLE = ((256, 200), (512, 300), (512, 512), (16640, 16500), (64000, 64000))
FORMS = {256: 256, 1256: 128}          # tile form -> TM
K_SOFT, K_OFF, K_IND = 4, 4, 5
W0_FILLS = (float("inf"), float("-inf"), float("nan"), 3e38)
INF = float("inf")


def _case(name, N, ce_cols, **kw):
    d = dict(name=name, N=N, ce_cols=ce_cols, K=64, B=4, S=60, lengths=(60, 1, 37, 52), row_start=None, exact=True)
    d.update(kw)
    return NS(**d)


CASES = {f"n{N}c{c}": _case(f"n{N}c{c}", N, c) for N, c in TABLE}
CASES["packed"] = _case("packed", 512, 300, B=2, S=120, lengths=(101, 1), row_start=(0, 128, 256))
CASES["gauss"] = _case("gauss", 512, 300, K=192, exact=False)


def row_layout(lengths, B, S, row_start=None, rows=M):
    """(valid [rows] bool, length of the row's sample [rows], 0 on rows of weight 0)."""
    valid, ln = torch.zeros(rows, dtype=torch.bool), torch.zeros(rows, dtype=torch.int64)
    for b in range(B):
        n = max(1, min(int(lengths[b]), S))
        r0 = row_start[b] if row_start is not None else b * S
        valid[r0:r0 + n], ln[r0:r0 + n] = True, n
    return valid, ln


def positions(N, ce_cols):
    """The indicator columns of a case, by what they reach in token_ce_merge_row (lane = tile % 64)."""
    nt = N // 256
    if nt >= 250:
        second, last, low = 69, 197, 5        # lane 5 owns tiles 5, 69, 133, 197
    elif nt >= 65:
        second, last, low = 64, 64, 0         # lane 0 owns tiles 0 and 64
    else:
        second, last, low = nt - 1, nt - 1, 0
    col = lambda t, o: min(t * 256 + o, ce_cols - 2)
    return {"tile0": 3, "tile0b": 67, "lastcol": ce_cols - 1, "second": col(second, 17), "lastiter": col(last, 140),
            "low": col(low, 200)}


def specs(N, ce_cols):
    """(class, {indicator: coefficient}, coefficient of the offset profile, target column or None = seeded) per row class."""
    p = positions(N, ce_cols)
    out = [("soft/t=any", {}, 5, None), ("soft/t=col0", {}, 5, 0), ("soft/t=last", {}, 5, ce_cols - 1),
           ("soft/t=strip31", {}, 5, 31), ("soft/t=strip95", {}, 5, 95)]
    if ce_cols > 256:
        out += [("soft/t=255", {}, 5, 255), ("soft/t=256", {}, 5, 256)]
    for k in ("tile0", "lastcol", "second", "lastiter", "low"):
        out += [(f"sharp32@{k}/t=winner", {k: 2}, 5, p[k]), (f"sharp80@{k}/t=winner", {k: 5}, 5, p[k]),
                (f"sharp128@{k}/t=underflowing", {k: 8}, 5, 1)]
    out += [("offset+80/t=any", {}, 10, None), ("offset+80/t=col0", {}, 10, 0), ("offset-80/t=any", {}, 0, None),
            ("offset-80/t=last", {}, 0, ce_cols - 1)]
    two = {"tile0": 2, "second": 2}
    out += [("tie2tiles/t=first", two, 5, p["tile0"]), ("tie2tiles/t=second", two, 5, p["second"]), ("tie2tiles/t=other", two, 5, 2)]
    one = {"tile0": 2, "tile0b": 2}
    out += [("tie1tile/t=second", one, 5, p["tile0b"]), ("tie1tile/t=other", one, 5, 2)]
    return out


def build(case):
    """The operands of a case, made on the CPU and seeded: NS(A bf16 [M,K], W bf16 [N,K], bias fp32 [N], tgt int64 [M],
    cls [M] names, valid, ln, dz (None when exact, else the float64 [M,N] bound on the logit error), floor_designed)."""
    N, cc, K = case.N, case.ce_cols, case.K
    g = torch.Generator().manual_seed(N * 7 + cc)
    valid, ln = row_layout(case.lengths, case.B, case.S, case.row_start)
    A = torch.zeros(M, K)
    tgt = torch.zeros(M, dtype=torch.int64)
    cls = [""] * M
    floor_designed = 0
    if case.exact:
        pos = positions(N, cc)
        keys = list(pos)
        W = torch.randint(-8, 9, (N, K), generator=g).float() * UNIT
        W[:, K_OFF] = 16.0
        W[:, K_IND:K_IND + len(keys)] = 0.0
        bias = -80.0 + torch.randint(-4, 5, (N,), generator=g).float() * UNIT
        bias[cc:] = 1000.0
        for j, k in enumerate(keys):
            W[pos[k], :K_SOFT] = 0.0
            W[pos[k], K_IND + j] = 16.0
            bias[pos[k]] = -80.0
        sp = specs(N, cc)
        for i, r in enumerate(valid.nonzero().flatten().tolist()):
            name, ind, off, t = sp[i % len(sp)]
            A[r, (i // len(sp)) % K_SOFT] = 1.0
            A[r, K_OFF] = float(off)
            for k, a in ind.items():
                A[r, K_IND + keys.index(k)] = float(a)
            tgt[r] = int(torch.randint(0, cc, (1,), generator=g)) if t is None else t
            cls[r] = name
            gap = 16 * max(ind.values()) if ind else 0
            if gap > 70:                     # exp(-gap) < 2^-100: every class but the winner's and a losing target's; a winning
                floor_designed += cc - (2 if tgt[r] != pos[next(iter(ind))] else 0)      # target's own w (1 - p) is below 2^-53 w
        dz = None
    else:
        A[valid] = torch.randn(int(valid.sum()), K, generator=g)
        W = torch.randn(N, K, generator=g) * 0.3
        bias = torch.randn(N, generator=g)
        bias[cc:] = 50.0
        tgt[valid] = torch.randint(0, cc, (int(valid.sum()),), generator=g)
        for r in valid.nonzero().flatten().tolist():
            cls[r] = "gauss"
    w0_t = (-1, cc, N + 5, 2 ** 40)
    for i, r in enumerate((~valid).nonzero().flatten().tolist()):
        A[r, :] = W0_FILLS[i % 4]
        tgt[r] = w0_t[(i // 4) % 4]
        cls[r] = f"weight0/A={W0_FILLS[i % 4]}/t={w0_t[(i // 4) % 4]}"
    A, W = A.to(torch.bfloat16), W.to(torch.bfloat16)
    if not case.exact:
        Av = torch.where(valid[:, None], A.double(), torch.zeros(1, dtype=torch.float64))
        dz = (K + 3) * 2.0 ** -23 * (Av.abs() @ W.double().abs().T + bias.double().abs())
    return NS(A=A, W=W, bias=bias, tgt=tgt, cls=cls, valid=valid, ln=ln, dz=dz, floor_designed=floor_designed)


@functools.lru_cache(maxsize=None)
def made(name):
    """(case, operands, float64 reference, allowances) of one table row: made once, shared by every test, left unchanged."""
    case = CASES[name]
    ops = build(case)
    ref = reference(ops.A, ops.W, ops.bias, ops.tgt, case.lengths, case.B, case.S, case.ce_cols, case.row_start)
    return case, ops, ref, allowances(ref, ops.dz)


@functools.lru_cache(maxsize=None)
def modelled(name, TM):
    """check()'s report on the restatement of one table row: the `model` column beside the kernels' fractions."""
    case, ops, ref, allow = made(name)
    got = restated(ops.A, ops.W, ops.bias, ops.tgt, case.lengths, case.B, case.S, case.ce_cols, TM, case.row_start, exact=case.exact)
    return check(got, ref, allow, ops.cls, case.exact)


def premise(ops):
    """The largest sum of the terms' magnitudes over the valid rows, in units of UNIT: below 2^24 every partial sum of
    every logit, in any order, is an exact fp32 number."""
    s = ops.A[ops.valid].double().abs() @ ops.W.double().abs().T + ops.bias.double().abs()
    return float(s.max()) / UNIT


def _logits64(A, W, bias, valid):
    z = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float64)
    z[valid] = A[valid].double() @ W.double().T + bias.double()
    return z


def reference(A, W, bias, tgt, lengths, B, S, ce_cols, row_start=None):
    """float64: NS(z logits (0 on rows of weight 0), tmax / tsum [M, ntile] per 256-column tile over the real classes
    ((-inf, 0) on a tile without one), lse, w (fp32: 1 / (B len), 0 on rows of weight 0), loss, grad = w (softmax - onehot)
    with zeros on rows of weight 0 and columns >= ce_cols, p the softmax, top1 = (valid rows, rows whose target logit
    equals the row maximum: plb_launch_token_top1's tie-inclusive rule), valid, tgt)."""
    Mr, N = A.shape[0], W.shape[0]
    valid, ln = row_layout(lengths, B, S, row_start, Mr)
    z = _logits64(A, W, bias, valid)
    zr = z.clone()
    zr[:, ce_cols:] = -INF
    zt = zr.reshape(Mr, N // 256, 256)
    tmax = zt.amax(2)
    tsum = torch.where(tmax[..., None] > -INF, torch.exp(zt - tmax[..., None].clamp_min(-1e300)), torch.zeros(1, dtype=torch.float64)).sum(2)
    lse = torch.logsumexp(zr, 1)
    w = torch.where(valid, 1.0 / (float(B) * ln.clamp_min(1).float()), torch.zeros(1))          # fp32 division, as the kernel's
    t = tgt.clamp(0, ce_cols - 1)
    z_t = z.gather(1, t[:, None])[:, 0]
    wd = w.double()
    loss = torch.where(valid, wd * (lse - z_t), torch.zeros(1, dtype=torch.float64))
    p = torch.exp(zr - lse[:, None]) * valid[:, None]
    grad = p * wd[:, None]
    rows = valid.nonzero().flatten()
    grad[rows, t[rows]] -= wd[rows]
    hits = int((valid & (z_t == zr.amax(1))).sum())
    return NS(z=z, tmax=tmax, tsum=tsum, lse=torch.where(valid, lse, torch.zeros(1, dtype=torch.float64)), w=w, loss=loss, grad=grad,
              p=p, z_t=z_t, top1=(int(valid.sum()), hits), valid=valid, tgt=tgt, ce_cols=ce_cols)


def e_exp(x):
    x = x.abs()
    return (x * LOG2E + 1.0) * 2.0 ** -23 + x * U


def allowances(ref, dz=None):
    """NS(psum [M, ntile] relative, lse [M], loss [M], grad [M, N], floor [M, N] bool) from the reference alone (module docstring)."""
    Mr, N = ref.z.shape
    cc, valid, wd = ref.ce_cols, ref.valid, ref.w.double()
    zr = ref.z.clone()
    zr[:, cc:] = INF
    tmin = zr.reshape(Mr, N // 256, 256).amin(2)
    has = ref.tmax > -INF
    zero = torch.zeros(1, dtype=torch.float64)
    dzr = dz.amax(1) if dz is not None else torch.zeros(Mr, dtype=torch.float64)
    psum = 256 * U + e_exp(torch.where(has, ref.tmax - tmin, zero)) + 2 * dzr[:, None]
    Mx = ref.tmax.amax(1)
    d = torch.where(has, (ref.tmax - Mx[:, None]).abs(), zero)
    lnl = ref.lse - torch.where(valid, Mx, zero)
    share = torch.where(has, ref.tsum * torch.exp(-d - lnl[:, None]), zero)
    dl = (share * (psum + d * (LOG2E * 2.0 ** -23 + U))).sum(1) + 10 * (2.0 ** -23 + 2 * U) + 10 * U
    dl = dl + lnl.abs() * 2.0 ** -22 + U * ref.lse.abs() + dzr
    dz_t = dz.gather(1, ref.tgt.clamp(0, cc - 1)[:, None])[:, 0] if dz is not None else 0.0
    loss = wd * (dl + 2.0 ** -23 * (ref.lse.abs() + ref.z_t.abs()) + dz_t)
    wp = wd[:, None] * ref.p
    grad = spacing_bf16(ref.grad) + wp * (dl[:, None] + (dz if dz is not None else 0.0) + e_exp(ref.z - ref.lse[:, None])) + U * wp
    rows = valid.nonzero().flatten()
    grad[rows, ref.tgt[rows]] += U * wd[rows]
    floor = (ref.grad.abs() < wd[:, None] * FLOOR) & valid[:, None]
    floor[:, cc:] = False
    return NS(psum=psum, lse=dl, loss=loss, grad=grad, floor=floor, dz=dz, dz_row=dzr)


def floor_count(ref):
    """How many gradient elements of real classes on valid rows the reference puts below w 2^-100."""
    f = (ref.grad.abs() < ref.w.double()[:, None] * FLOOR) & ref.valid[:, None]
    return int(f[:, :ref.ce_cols].sum())


# ---------------------------------------------------------------------------------------------------------- restatement
def _pair(m1, s1, m2, s2):
    """One step of the kernels' (max, sum) merges: sm = mm > -inf ? s1 exp(m1 - mm) + s2 exp(m2 - mm) : 0."""
    mm = torch.maximum(m1, m2)
    safe = torch.where(mm > -INF, mm, torch.zeros_like(mm))
    return mm, torch.where(mm > -INF, s1 * torch.exp(m1 - safe) + s2 * torch.exp(m2 - safe), torch.zeros_like(s1))


def merge_rows(pmax, psum, defect=None):
    """token_ce_merge_row in fp32 on [rows, ntiles] pairs: lane i % 64 walks tiles i, i + 64, ... keeping (m, l) with the
    rescale `if (pm > m) l *= exp(m - pm)`; then M = the lanes' maximum, l = butterfly sum of l exp(m - M) (0 for a lane
    that saw no finite maximum), lse = M + log(l). defect: ("drop", row) leaves lane 0's second tile out, ("norescale", row)
    omits the rescale in a lane's later iterations."""
    R, nt = pmax.shape
    it = -(-nt // 64)
    pm = torch.full((R, it * 64), -INF)
    ps = torch.zeros(R, it * 64)
    pm[:, :nt], ps[:, :nt] = pmax.float(), psum.float()
    present = (torch.arange(it * 64) < nt).reshape(it, 64)
    pm, ps = pm.reshape(R, it, 64), ps.reshape(R, it, 64)
    m, l = torch.full((R, 64), -INF), torch.zeros(R, 64)
    for i in range(it):
        pr = present[i][None, :].expand(R, 64).clone()
        if defect and defect[0] == "drop" and i == 1:
            pr[defect[1], 0] = False
        gt = pr & (pm[:, i] > m)
        resc = l * torch.exp(torch.where(gt, m - pm[:, i], torch.zeros(1)))
        if defect and defect[0] == "norescale" and i >= 1:
            resc[defect[1]] = l[defect[1]]
        l = torch.where(gt, resc, l)
        m = torch.where(gt, pm[:, i], m)
        add = pr & (pm[:, i] > -INF)
        l = torch.where(add, l + ps[:, i] * torch.exp(torch.where(add, pm[:, i] - m, torch.zeros(1))), l)
    Mw = m.amax(1)
    t = torch.where(m == -INF, torch.zeros(1), l * torch.exp(torch.where(m == -INF, torch.zeros(1), m - Mw[:, None])))
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        t = t + t[:, idx ^ o]
    return Mw + torch.log(t[:, 0])


def restated(A, W, bias, tgt, lengths, B, S, ce_cols, TM, row_start=None, defect=None, exact=True):
    """The kernels' own algorithm in fp32 on the CPU (torch's exp / log): the model of what a correct kernel computes.
    Pass 1: per lane the maximum of its 16 values of a 256-column tile and the sum of exp(z - max) in the epilogue's order,
    the four-lane butterfly, the four-wave chain; the merge (merge_rows); pass 2: exp(z - lse) w - (c == t ? w : 0) rounded
    to bf16 (RNE); colpart: per (row tile, wave half) the fp32 column sums of the stored values; the top-1 totals.
    defect = (name, row): the seeded defects of tests/test_token_ce_host.py. Returns NS in launch()'s layout."""
    Mr, N = A.shape[0], W.shape[0]
    nt = N // 256
    valid, ln = row_layout(lengths, B, S, row_start, Mr)
    rows = valid.nonzero().flatten()
    dname, drow = defect if defect else (None, None)
    if exact:
        z = (A[rows].double() @ W.double().T + bias.double()).float()
    else:
        z = A[rows].float() @ W.float().T + bias
    R = len(rows)
    vi = {int(r): i for i, r in enumerate(rows.tolist())}     # row -> index among the valid rows
    t = tgt[rows]
    cols1 = ce_cols + (1 if dname == "cols+1" else 0)
    zr = z.clone()
    zr[:, cols1:] = -INF
    zl = zr.reshape(R, nt, 2, 4, 2, 4, 4)                       # column = nh 128 + wn 32 + ni 16 + fq 4 + r
    mx = zl.amax((2, 4, 6))                                     # [R, nt, wn, fq]
    mb = mx[:, :, None, :, None, :, None]
    e = torch.where(mb > -INF, torch.exp(zl - torch.where(mb > -INF, mb, torch.zeros(1))), torch.zeros(1))
    q = (e[..., 0] + e[..., 1]) + (e[..., 2] + e[..., 3])       # [R, nt, nh, wn, ni, fq]
    sm = torch.zeros(R, nt, 4, 4)
    for nh in range(2):
        for ni in range(2):
            sm = sm + q[:, :, nh, :, ni, :]
    m01, s01 = _pair(mx[..., 0], sm[..., 0], mx[..., 1], sm[..., 1])
    m23, s23 = _pair(mx[..., 2], sm[..., 2], mx[..., 3], sm[..., 3])
    mw, sw = _pair(m01, s01, m23, s23)                          # [R, nt, wn]
    pm, ps = torch.full((R, nt), -INF), torch.zeros(R, nt)
    for w4 in range(4):
        pm, ps = _pair(pm, ps, mw[..., w4], sw[..., w4])
    tl = z[torch.arange(R), t]
    md = None
    if dname in ("drop", "norescale"):
        md = (dname, vi[drow])
    lse = merge_rows(pm, ps, md)
    wt = 1.0 / (float(B) * ln[rows].float())
    loss = wt * (lse - tl)
    lse2 = lse.clone()
    if dname == "neighbour_lse":
        lse2[vi[drow]] = lse[vi[drow] + 1]
    g = torch.where(torch.arange(N)[None, :] < ce_cols, torch.exp(z - lse2[:, None]) * wt[:, None], torch.zeros(1))
    if dname == "softmax*1.03":
        g[vi[drow]] *= 1.03
    hot = t.clone()
    if dname == "onehot+1":
        hot[vi[drow]] += 1
    g[torch.arange(R), hot] -= wt
    out = NS(TM=TM)
    out.pmax, out.psum = torch.zeros(Mr, nt), torch.zeros(Mr, nt)
    out.pmax[rows], out.psum[rows] = pm, ps
    out.tlogit = torch.full((Mr,), float("nan"))
    out.tlogit[rows] = tl
    out.lse, out.w, out.loss = torch.zeros(Mr), torch.zeros(Mr), torch.zeros(Mr)
    out.lse[rows], out.w[rows], out.loss[rows] = lse, wt, loss
    out.grad = torch.zeros(Mr, N, dtype=torch.bfloat16)
    out.grad[rows] = g.to(torch.bfloat16)
    if dname == "0*exp(inf)":
        out.grad[drow, :ce_cols] = float("nan")                # 0 * exp(+inf - lse)
    st = out.grad.float()
    half = (torch.arange(Mr) % 128) // 64
    out.colpart = torch.zeros(2 * (Mr // TM), N)
    for rt in range(Mr // TM):
        for wm in range(2):
            sel = (torch.arange(Mr) // TM == rt) & (half == wm)
            if dname == "colpart-64" and drow == 2 * rt + wm:
                sel &= torch.arange(Mr) % TM >= 64 * (wm + 1)   # the first of this half's 64-row blocks is missing
            out.colpart[2 * rt + wm] = st[sel].sum(0)
    out.dbias = st.double().sum(0)[:ce_cols].float()
    out.loss_sum = float(out.loss.double().sum())
    rowmax = pm.amax(1)
    hit = tl == rowmax
    if dname == "tie_not_top1":                                 # the lowest-index rule: of equal maxima only the first counts
        hit &= t == zr.argmax(1)
    out.totals = (R, int(hit.sum()))
    return out


def merge_reference(pmax, psum):
    """float64 log-sum-exp of [rows, ntiles] (max, sum) pairs and d_lse without the psum term (the pairs are inputs here)."""
    pm, ps = pmax.double(), psum.double()
    Mx = pm.amax(1)
    has = pm > -INF
    zero = torch.zeros(1, dtype=torch.float64)
    d = torch.where(has, (pm - Mx[:, None]).abs(), zero)
    l = torch.where(has, ps * torch.exp(-d), zero).sum(1)
    lse = Mx + torch.log(l)
    share = torch.where(has, ps * torch.exp(-d), zero) / l[:, None]
    dl = (share * d * (LOG2E * 2.0 ** -23 + U)).sum(1) + 10 * (2.0 ** -23 + 2 * U) + 10 * U + torch.log(l).abs() * 2.0 ** -22 + U * lse.abs()
    return lse, dl


MERGE_NTILES = (1, 4, 64, 65, 250)


def merge_pairs(nt):
    """Synthetic [15, nt] (max, sum) pairs for the merge kernels alone: maxima spread over +-80, ascending / descending by
    tile (so within every lane) and three random orders, each plain, with a (-inf, 0) pair as tile 0 (a lane's FIRST tile)
    and with one as a later tile of the same lane (tile 64; the last tile when lanes own one tile each). Sums in [1, 256]."""
    g = torch.Generator().manual_seed(500 + nt)
    asc = torch.linspace(-80.0, 80.0, nt) if nt > 1 else torch.tensor([3.0])
    orders = [asc, asc.flip(0)] + [asc[torch.randperm(nt, generator=g)] for _ in range(3)]
    pm, ps = [], []
    for o in orders:
        for hole in (None, 0, 64 if nt > 64 else nt - 1):
            m, s = o.clone(), torch.rand(nt, generator=g) * 255 + 1
            if hole is not None and nt > 1:
                m[hole], s[hole] = -INF, 0.0
            pm.append(m)
            ps.append(s)
    return torch.stack(pm), torch.stack(ps)


# -------------------------------------------------------------------------------------------------------------- checker
def check(got, ref, allow, cls, exact=True):
    """Every output element of `got` (launch()'s or restated()'s layout) against the reference under allowances(). Returns
    {output: NS(bad, first, row, col, frac, at)}: how many elements are outside, the first one in words (row, row tile, column
    tile, column, class of the row, both values) and as (row, col), the largest fraction of the allowance used and where.
    Outputs with an exact contract report frac 0 or inf."""
    TM, valid, cc = got.TM, ref.valid, ref.ce_cols
    Mr, N = ref.z.shape
    rep = {}

    def put(name, excess, g, w, kind="element"):
        """excess: |error| / allowance per element (nan counts as outside). kind: what the two indices of an element are."""
        ex = torch.where(torch.isnan(excess), torch.full_like(excess, INF), excess.double())
        if ex.dim() == 1:
            ex, g, w = ex[:, None], g[:, None], w[:, None]
        bad = ex > 1.0

        def words(rr, c):
            where_ = {"element": f"row {rr} (row tile {rr // TM}), column {c} (column tile {c // 256})",
                      "tile": f"row {rr} (row tile {rr // TM}), column tile {c}", "row": f"row {rr} (row tile {rr // TM})",
                      "pair": f"colpart rows {2 * rr}, {2 * rr + 1} (row tile {rr}), column {c} (column tile {c // 256})",
                      "column": f"column {c} (column tile {c // 256})", "scalar": "the scalar"}[kind]
            tag = f" [{cls[rr]}]" if kind in ("element", "tile", "row") else ""
            return f"{where_}{tag}: got {float(g[rr, c])!r}, want {float(w[rr, c])!r}"

        r = NS(bad=int(bad.sum()), first=None, row=None, col=None, frac=float(ex.max()), at=None)
        rr, c = (int(v) for v in (ex == ex.max()).nonzero()[0])
        r.at = words(rr, c)
        if r.bad:
            r.row, r.col = (int(v) for v in bad.nonzero()[0])
            r.first = f"{r.bad} of {bad.numel()} outside; first at " + words(r.row, r.col)
        rep[name] = r

    def exact_eq(a, b):
        return torch.where(a.double() == b.double(), 0.0, INF).double()

    v2 = valid[:, None]
    # pass 1
    if exact:
        ex = exact_eq(got.pmax, ref.tmax)
        ext = exact_eq(got.tlogit, ref.z_t)
    else:
        fin = ref.tmax > -INF
        ex = torch.where(fin, (got.pmax.double() - ref.tmax).abs() / allow.dz_row[:, None].clamp_min(1e-300), exact_eq(got.pmax, ref.tmax))
        ext = (got.tlogit.double() - ref.z_t).abs() / allow.dz_row.clamp_min(1e-300)
    put("pmax", torch.where(v2, ex, torch.zeros(1, dtype=torch.float64)), got.pmax, ref.tmax, "tile")
    put("tlogit", torch.where(valid, ext, torch.zeros(1, dtype=torch.float64)), got.tlogit, ref.z_t, "row")
    empty = ref.tmax == -INF
    exs = torch.where(empty, exact_eq(got.psum, ref.tsum), (got.psum.double() - ref.tsum).abs() / (allow.psum * ref.tsum).clamp_min(1e-300))
    put("psum", torch.where(v2, exs, torch.zeros(1, dtype=torch.float64)), got.psum, ref.tsum, "tile")
    # merge
    zero1 = torch.zeros(Mr, dtype=torch.float64)
    for name, g, w, a in (("lse", got.lse, ref.lse, allow.lse), ("loss", got.loss, ref.loss, allow.loss)):
        exm = torch.where(valid, (g.double() - w).abs() / a.clamp_min(1e-300), exact_eq(g, zero1))
        put(name, exm, g, w, "row")
    put("w", exact_eq(got.w, ref.w), got.w, ref.w, "row")
    # pass 2
    gg = got.grad.double()
    exg = (gg - ref.grad).abs() / allow.grad.clamp_min(1e-300)
    wfl = (ref.w.double() * FLOOR)[:, None].expand(Mr, N)
    exg = torch.where(allow.floor, gg.abs() / wfl.clamp_min(1e-300), exg)
    must0 = ~v2.expand(Mr, N).clone()
    must0[:, cc:] = True
    exg = torch.where(must0, exact_eq(gg, torch.zeros(1, dtype=torch.float64).expand(Mr, N)), exg)
    put("grad", exg, got.grad, ref.grad)
    # column sums of the stored rows
    st = got.grad.double()
    st = torch.where(torch.isnan(st), torch.zeros(1, dtype=torch.float64), st)      # (reported under grad; keep the sums' verdict apart)
    pair = got.colpart.double().reshape(Mr // TM, 2, N).sum(1)
    want = st.reshape(Mr // TM, TM, N).sum(1)
    mag = st.abs().reshape(Mr // TM, TM, N).sum(1)
    exc = torch.where(mag > 0, (pair - want).abs() / ((TM // 2 + 1) * U * mag).clamp_min(1e-300), exact_eq(pair, torch.zeros_like(pair)))
    put("colpart", exc, pair, want, "pair")
    if getattr(got, "dbias", None) is not None:
        depth = TM // 2 + 1 + got.colpart.shape[0] + 11
        wantb, magb = st.sum(0)[:cc], st.abs().sum(0)[:cc]
        exb = torch.where(magb > 0, (got.dbias.double() - wantb).abs() / (depth * U * magb).clamp_min(1e-300), exact_eq(got.dbias, wantb))
        put("dbias", exb[None, :], got.dbias[None, :], wantb[None, :], "column")
    if getattr(got, "loss_sum", None) is not None:
        depth = -(-Mr // 256) + 9                 # plb_launch_sum_rows: per-thread chain, wave butterfly, 4 wave sums (test_gpu_rowops.py)
        wants = float(got.loss.double().sum())
        exsum = abs(got.loss_sum - wants) / max(depth * U * float(got.loss.double().abs().sum()), 1e-300)
        put("loss_sum", torch.tensor([exsum if exsum == exsum else INF]), torch.tensor([got.loss_sum]), torch.tensor([wants]), "scalar")
    ok = tuple(got.totals) == tuple(ref.top1)
    rep["top1"] = NS(bad=0 if ok else 1, row=None, col=None, frac=0.0 if ok else INF, at=f"totals2 {tuple(got.totals)}",
                     first=None if ok else f"totals2 (valid rows, tie-inclusive top-1 rows): got {tuple(got.totals)}, want {tuple(ref.top1)}")
    return rep


def failures(rep):
    return [f"{k}: {v.first}" for k, v in rep.items() if v.bad]


def fractions(rep):
    return {k: v.frac for k, v in rep.items()}


# --------------------------------------------------------------------------------------------------------------- launch
def launch(ops, case, form, dev="cuda", packed_merge=None):
    """The whole chain on the device, outputs prefilled with NaN: act 3, the merge (packed when the case has a plan;
    packed_merge=False runs the PADDED merge on such a case with S = 128, where row b 128 + s is the plan's row), then
    plb_launch_sum_rows, act 4 with colpart, plb_launch_colsum, plb_launch_token_top1. Returns the outputs on the CPU in
    restated()'s layout."""
    import ctypes as C
    from plbert_amd import _lib
    from gpu_util import stream
    L = _lib.lib()
    N, K, cc, B, S = case.N, case.K, case.ce_cols, case.B, case.S
    TM, nt = FORMS[form], case.N // 256
    nan = float("nan")
    A, W, bias, tgt = ops.A.to(dev), ops.W.to(dev), ops.bias.to(dev), ops.tgt.to(dev)
    lengths = torch.tensor(case.lengths, dtype=torch.int32, device=dev)
    packed = case.row_start is not None if packed_merge is None else packed_merge
    if case.row_start is not None and not packed:
        assert all(r == 128 * b for b, r in enumerate(case.row_start)) and M == 128 * B
        S = 128
    plan = torch.tensor(case.row_start, dtype=torch.int32, device=dev) if case.row_start is not None else None
    f = lambda *s: torch.full(s, nan, device=dev)
    pmax, psum, tl, lse, w, loss = f(M, nt), f(M, nt), f(M), f(M), f(M), f(M)
    dl = torch.full((M, N), nan, dtype=torch.bfloat16, device=dev)
    cprows = 2 * (M // TM)
    colp, dbias, scratch, lsum = f(cprows, N), f(cc), f(N), f(1)
    tscr = torch.full((2 * ((M + 3) // 4),), -7, dtype=torch.int32, device=dev)
    totals = torch.full((2,), -7, dtype=torch.int32, device=dev)
    p = _lib.PlbGemmNT()
    p.A, p.lda, p.B, p.ldb, p.M, p.N, p.K, p.Mstore = A.data_ptr(), K, W.data_ptr(), K, M, N, K, M
    p.bias, p.ce_cols, p.ce_tgt = bias.data_ptr(), cc, tgt.data_ptr()
    p.ce_pmax, p.ce_psum, p.ce_tlogit = pmax.data_ptr(), psum.data_ptr(), tl.data_ptr()
    assert L.plb_launch_gemm_nt_big(C.byref(p), form, 3, 0, stream()) == 0
    if packed:
        assert L.plb_launch_token_ce_combine_packed(pmax.data_ptr(), psum.data_ptr(), nt, tl.data_ptr(), lengths.data_ptr(),
                                                    plan.data_ptr(), B, S, M, lse.data_ptr(), w.data_ptr(), loss.data_ptr(), stream()) == 0
    else:
        assert L.plb_launch_token_ce_combine(pmax.data_ptr(), psum.data_ptr(), nt, tl.data_ptr(), lengths.data_ptr(), B, S, M,
                                             lse.data_ptr(), w.data_ptr(), loss.data_ptr(), stream()) == 0
    assert L.plb_launch_sum_rows(loss.data_ptr(), M, lsum.data_ptr(), stream()) == 0
    p.ce_lse, p.ce_w, p.C, p.ldc, p.colpart = lse.data_ptr(), w.data_ptr(), dl.data_ptr(), N, colp.data_ptr()
    assert L.plb_launch_gemm_nt_big(C.byref(p), form, 4, 0, stream()) == 0
    assert L.plb_launch_colsum(colp.data_ptr(), 0, cprows, N, N, dbias.data_ptr(), cc, 0, scratch.data_ptr(), 1, stream()) == 0
    assert L.plb_launch_token_top1(pmax.data_ptr(), nt, tl.data_ptr(), w.data_ptr(), M, tscr.data_ptr(), totals.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    out = NS(TM=TM, pmax=pmax.cpu(), psum=psum.cpu(), tlogit=tl.cpu(), lse=lse.cpu(), w=w.cpu(), loss=loss.cpu(), grad=dl.cpu(),
             colpart=colp.cpu(), dbias=dbias.cpu(), loss_sum=float(lsum.item()), totals=tuple(int(v) for v in totals.cpu()))
    return out


def same_bits(a, b, rows=None):
    """Names of the outputs of two launch() results that differ in any bit (on `rows` of the per-row outputs when given)."""
    bad = []
    for k in ("pmax", "psum", "lse", "w", "loss", "grad", "colpart", "dbias"):
        x, y = getattr(a, k), getattr(b, k)
        if rows is not None and x.shape[0] == rows.shape[0]:
            x, y = x[rows], y[rows]
        iv = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
        if not torch.equal(x.contiguous().view(iv), y.contiguous().view(iv)):
            bad.append(k)
    if a.totals != b.totals:
        bad.append("totals")
    if rows is None and a.loss_sum != b.loss_sum:
        bad.append("loss_sum")
    return bad
