"""Helpers shared by the -m gpu tests: raw launches through the C ABI with torch tensors as buffers."""
import ctypes as C

import pytest
import torch

from plbert_amd import _lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def rel_l2(a, b):
    a = a.double().flatten()
    b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


_byref = C.byref


def _out(M, ld, dtype, dev, fill):
    return torch.zeros((M, ld), dtype=dtype, device=dev) if fill is None else torch.full((M, ld), fill, dtype=dtype, device=dev)


def gemm_nt(A, B, N, bias=None, res=None, aux=None, act=0, out_f32=False, Mstore=None, ldout=None, *, lda=None, ldb=None,
            ldc=None, ldc2=None, ldcf=None, ldr=None, ldaux=None, C=None, colpart=None, fill=None):
    """A [M,K] bf16, B [>=ceil128(N),K] bf16 -> C (bf16 or fp32) [M, ldout].
    Leading dimensions: the inputs' default to their row strides (a column slice of a wider buffer is a strided operand),
    the outputs' to ldout; each can be given per buffer. C: a caller-provided bf16 output [M, ldc] (the in-place case: the
    buffer `res` is a view of); colpart: an fp32 buffer for the big-tile kernels' column-sum partials; fill: the value the
    outputs this function allocates hold before the launch (default zeros). Returns the whole [M, ld] buffers."""
    L = _lib.lib()
    M, K = A.shape
    ldout = ldout or N
    dev = A.device
    ldc = ldc or (C.stride(0) if C is not None else ldout)
    Cb = C if C is not None else _out(M, ldc, torch.bfloat16, dev, fill)
    C2 = _out(M, ldc2 or ldout, torch.bfloat16, dev, fill)
    Cf = _out(M, ldcf or ldout, torch.float32, dev, fill)
    p = _lib.PlbGemmNT()
    p.A, p.lda, p.B, p.ldb = A.data_ptr(), lda or A.stride(0), B.data_ptr(), ldb or B.stride(0)
    p.M, p.N, p.K, p.Mstore = M, N, K, (M if Mstore is None else Mstore)
    p.bias = bias.data_ptr() if bias is not None else None
    if res is not None:
        p.res, p.ldr = res.data_ptr(), ldr or res.stride(0)
    if aux is not None:
        p.aux, p.ldaux = aux.data_ptr(), ldaux or aux.stride(0)
    p.C, p.ldc, p.C2, p.ldc2, p.Cf, p.ldcf = Cb.data_ptr(), ldc, C2.data_ptr(), C2.stride(0), Cf.data_ptr(), Cf.stride(0)
    if colpart is not None:
        p.colpart = colpart.data_ptr()
    rc = L.plb_launch_gemm_nt(_byref(p), act, int(out_f32), stream())   # (the parameter C shadows ctypes here)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return (Cf if out_f32 else Cb), C2


def gemm_tn(A, B, N, splits, rows_per_split, big=False):
    """A [Mtot, Ncols] bf16, B [Mtot, K] bf16 -> dW [N,K] fp32 (slabs reduced)."""
    L = _lib.lib()
    Mtot, Ncols = A.shape
    K = B.shape[1]
    slab = torch.zeros((splits, N, K), dtype=torch.float32, device=A.device)
    out = torch.zeros((N, K), dtype=torch.float32, device=A.device)
    p = _lib.PlbGemmTN()
    p.A, p.lda, p.Ncols, p.B, p.ldb = A.data_ptr(), A.stride(0), Ncols, B.data_ptr(), B.stride(0)
    p.Mtot, p.N, p.K, p.rows_per_split, p.splits, p.slab = Mtot, N, K, rows_per_split, splits, slab.data_ptr()
    if big:
        rc = L.plb_launch_gemm_tn_big(C.byref(p), stream())
    else:
        rc = L.plb_launch_gemm_tn(C.byref(p), stream())
    assert rc == 0, rc
    rc = L.plb_launch_reduce_slabs(slab.data_ptr(), splits, N * K, out.data_ptr(), 0, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def attn_args(qkv, lengths, B, S, NH):
    H = NH * 64
    dev = qkv.device
    p = _lib.PlbAttn()
    ctx = torch.zeros((B * S, H), dtype=torch.bfloat16, device=dev)
    lse = torch.zeros((B, NH, S), dtype=torch.float32, device=dev)
    p.qkv, p.ldqkv = qkv.data_ptr(), qkv.stride(0)
    p.lengths = lengths.data_ptr() if lengths is not None else None
    p.B, p.S, p.NH, p.H, p.scale = B, S, NH, H, 0.125
    p.ctx, p.ldctx, p.lse = ctx.data_ptr(), H, lse.data_ptr()
    return p, ctx, lse


def torch_attention(qkv, lengths, B, S, NH):
    """fp32 reference on the same (bf16-rounded) inputs; returns ctx [B*S,H], lse [B,NH,S], and a
    function computing dqkv for a given dctx."""
    H = NH * 64
    x = qkv.float().detach().clone().requires_grad_(True)
    q, k, v = [t.reshape(B, S, NH, 64).transpose(1, 2) for t in x.split(H, dim=1)]
    s = (q @ k.transpose(2, 3)) * 0.125
    if lengths is not None:
        keymask = torch.arange(S, device=qkv.device)[None, :] >= lengths[:, None].long()
        s = s.masked_fill(keymask[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    ctx = (p @ v).transpose(1, 2).reshape(B * S, H)

    def grad(dctx):
        (g,) = torch.autograd.grad(ctx, x, dctx.float())
        return g

    return ctx.detach(), lse.detach(), grad


def ptr_array(tensors, ctype=C.c_void_p):
    """A C array of device pointers (None stays NULL)."""
    return (ctype * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


# ---- the fp8 image contract ---------------------------------------------------------------------------------------------
# Every 1-byte image the kernels write is OCP-fp8(clamp(stored value x scale)): the value as it was stored (bf16, or the fp32
# source of plb_launch_quantize), multiplied by the site's scale in fp32, saturated to the format's largest finite value,
# rounded to nearest even. The reference is formed on the CPU by torch's OCP casts (pinned against fp8_np.round_fp8 in
# tests/test_oracle_fp8.py), independently of the device.
F8_SLOTS, F8_STRIDE = 64, 16   # one amax site: 64 words on separate 64-byte lines (csrc/common.h)


def fp8_fmax(bf8):
    return 57344.0 if bf8 else 448.0


def ocp_bytes(stored, scale, bf8):
    """The reference image of `stored` (bf16 or fp32) at `scale` (a float or a one-element tensor), as uint8 on the CPU."""
    s = torch.as_tensor(scale, dtype=torch.float32).detach().cpu().reshape(-1)[:1]
    mx = fp8_fmax(bf8)
    x = stored.detach().cpu().float() * s   # fp32 product, as the kernels form it
    return x.clamp(-mx, mx).to(torch.float8_e5m2 if bf8 else torch.float8_e4m3fn).view(torch.uint8)


def site_max(site):
    """Maximum over the 64 slots of one amax site."""
    return float(site.detach().reshape(F8_SLOTS, F8_STRIDE)[:, 0].max())


def assert_fp8_image(img_u8, stored, scale, bf8, rows, amax_site=None, sentinel=None, cols=None):
    """img_u8 [R, >=C] uint8 (the buffer the kernel wrote into), stored [<=R, >=C] the values it stored; rows: the rows (an
    index tensor, a slice or a boolean mask) the kernel stored. The bytes of those rows must equal the reference image bit
    for bit; with `sentinel`, every other byte of the buffer must still hold it. With `amax_site`, the site's maximum must
    EQUAL max |stored| over those rows (both are maxima of the same bf16 / fp32 values: no rounding separates them)."""
    img = img_u8.detach().cpu()
    st = stored.detach().cpu()
    cols = cols if cols is not None else st.shape[1]
    mask = torch.zeros(img.shape[0], dtype=torch.bool)
    mask[rows] = True
    assert not bool(mask[st.shape[0]:].any()), "stored rows past the stored tensor"
    smask = mask[:st.shape[0]]           # the image buffer may have rows past the stored tensor (they hold the sentinel)
    got = img[mask, :cols]
    want = ocp_bytes(st[smask, :cols], scale, bf8)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        r, c = (int(v) for v in bad[0])
        raise AssertionError(f"{len(bad)} image bytes differ; first at ({r}, {c}): got 0x{int(got[r, c]):02x}, want "
                             f"0x{int(want[r, c]):02x} for stored {float(st[smask][r, c].float())!r}")
    if sentinel is not None:
        outside = img.clone()
        outside[mask, :cols] = sentinel
        assert bool((outside == sentinel).all()), "image bytes outside the stored rows / columns were written"
    if amax_site is not None:
        want_max = float(st[smask, :cols].float().abs().max()) if bool(smask.any()) else 0.0
        assert site_max(amax_site) == want_max, (site_max(amax_site), want_max)


# ---- the attention row contract (tests/test_gpu_attention_rows.py, tests/test_attention_rows_host.py) ---------------------
# Every (token row, head) of ctx, dQ, dK and dV is held to the float64 evaluation of the same bf16 inputs, within 4 x the
# WORST row of a float64 evaluation that rounds only where the kernels round. Nothing below calls a kernel: the helpers run
# on whatever device the inputs live on, so the host file exercises them on the CPU.
ATTN_SCALE = 0.125     # head_dim 64 (attn_args)
ROW_FACTOR = 4.0       # kernel row error <= ROW_FACTOR x the model's worst row (fp32 summation order, hardware exp2, the
                       # forward's lazy rescale and the scatter of a finite sample's worst row: each second order to a
                       # bf16 rounding)
ROW_TINY = 1e-6        # a row whose float64 norm is below this fraction of the output's largest row norm is checked
ROW_ABS = 1e-5         # absolutely: |got| < ROW_ABS


@pytest.fixture
def bwd_form(request):
    """Forces the attention backward's form: 0 = dq + dkv kernels, 1 = the single-kernel form (S <= 512); afterwards the
    per-shape policy (-1) is back."""
    L = _lib.lib()
    L.plb_set_attn_bwd_fused(int(request.param))
    yield int(request.param)
    L.plb_set_attn_bwd_fused(-1)


def _r16(x):
    return x.to(torch.bfloat16).double()


def _attention_eval(qkv, lengths, B, S, NH, q, qoff, rounded):
    H = NH * 64
    dev = qkv.device
    x = qkv.double()
    heads = lambda t, n: t.reshape(B, n, NH, 64).permute(0, 2, 1, 3)          # [B*n, H] -> [B, NH, n, 64]
    rows = lambda t, n: t.permute(0, 2, 1, 3).reshape(B, n, H)                # and back, per sample
    K, V = heads(x[:, H:2 * H], S), heads(x[:, 2 * H:3 * H], S)
    lens = torch.full((B,), S, dtype=torch.long, device=dev) if lengths is None else lengths.long().clamp(1, S)
    masked = (torch.arange(S, device=dev)[None, :] >= lens[:, None])[:, None, None, :]   # keys past the length
    if qoff is None:
        Sq, Nq, qvalid = S, B * S, None
        Q = heads(x[:, :H], S)
    else:  # compact queries: sample b's queries are rows [qoff[b], qoff[b+1]) of q, padded here to the largest count
        off = qoff.long()
        counts = off[1:] - off[:-1]
        Nq, Sq = int(off[-1]), max(int(counts.max()), 1)
        pos = torch.arange(Sq, device=dev)[None, :]
        qvalid = pos < counts[:, None]                                        # [B, Sq]
        Qp = torch.zeros((B, Sq, H), dtype=torch.float64, device=dev)
        Qp[qvalid] = q.double()[:Nq, :H]                                      # row-major over (b, pos) = compact order
        Q = heads(Qp, Sq)
    pack = (lambda t: rows(t, Sq).reshape(B * Sq, H)) if qoff is None else (lambda t: rows(t, Sq)[qvalid])
    stat = (lambda t: t) if qoff is None else (lambda t: t.permute(1, 0, 2)[:, qvalid])   # [B,NH,S] | [NH,Nq]
    sraw = Q @ K.transpose(2, 3)                                              # raw scores [B, NH, Sq, S]
    s = (sraw * ATTN_SCALE).masked_fill(masked, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    lse = (m + torch.log(l)).squeeze(-1)
    if rounded:
        # forward: exp(s - reference) leaves the S accumulator as a bf16 MFMA operand (acc_frag), the row sum is taken
        # from the fp32 values, the division by it happens in fp32 at the end, and the context row is stored as bf16
        ctx = _r16((_r16(e) @ V) / l)
    else:
        ctx = (e / l) @ V

    def grad(dctx, ctx_stored=None):
        """dctx by (compact) query row -> dq by (compact) query row, dk, dv [B*S, H], delta in the layout of the
        statistics. delta = -sum(dO * O) over the context rows the kernel stored (ctx_stored) when given."""
        if qoff is None:
            dO = heads(dctx.double(), S)
        else:
            dOp = torch.zeros((B, Sq, H), dtype=torch.float64, device=dev)
            dOp[qvalid] = dctx.double()[:Nq]
            dO = heads(dOp, Sq)
        if rounded:
            # the backward recomputes P = exp2(c * S + bias) from the statistic the forward stored: fp32, minus the
            # log-sum-exp in units of raw scores; delta is the row sum of dO with the context AS STORED (bf16)
            lse_st = (-lse / ATTN_SCALE).float().double()
            P = torch.exp((sraw + lse_st[..., None]) * ATTN_SCALE).masked_fill(masked, 0.0)
        else:
            P = e / l
        delta = (dO * ctx).sum(-1, keepdim=True)
        dS = P * (dO @ V.transpose(2, 3) - delta)
        if rounded:
            dS = _r16(dS)                                                     # operand of dS.K and dS^T.Q (all forms)
        dq = (dS @ K) * ATTN_SCALE
        dk = (dS.transpose(2, 3) @ Q) * ATTN_SCALE
        dv = (_r16(P) if rounded else P).transpose(2, 3) @ dO                 # P as a bf16 operand of dV = P^T.dO
        if rounded:
            dq, dk, dv = _r16(dq), _r16(dk), _r16(dv)
        if ctx_stored is None:
            dl = -stat(delta.squeeze(-1))
        else:
            dl = attention_delta_terms(dctx, ctx_stored, B, S, NH, qoff)[0]
        return pack(dq), rows(dk, S).reshape(B * S, H), rows(dv, S).reshape(B * S, H), dl

    return pack(ctx), stat(lse), grad


def attention_fp64(qkv, lengths, B, S, NH, q=None, qoff=None):
    """float64 attention on the same (bf16-rounded) inputs: ctx [rows, H], lse (natural log, scaled scores) [B, NH, S] and
    grad(dctx, ctx_stored=None) -> (dq, dk, dv, delta). Compact-query mode follows PlbAttn.qoff: the queries are the rows
    of q, keys and values come from qkv; ctx, dq by compact row, lse and delta [NH, Nq]."""
    return _attention_eval(qkv, lengths, B, S, NH, q, qoff, False)


def attention_rounded(qkv, lengths, B, S, NH, q=None, qoff=None):
    """attention_fp64 with the roundings the kernels make (attn.hip, attn_bwd_fused.hip, attn_common.h) and float64 in
    between — the source of the row tolerance:
      forward   exp(s - reference) -> bf16 before P.V; the row sum and the final division stay unrounded; ctx -> bf16
      statistic minus log-sum-exp in raw-score units -> fp32 (PlbAttn.lse); the backward recomputes P from it
      backward  delta from the bf16 ctx; P -> bf16 before P^T.dO only; dS = P(dP - delta) -> bf16 before dS.K and dS^T.Q;
                dq, dk, dv -> bf16
    Both backward forms round at the same points (the single-kernel form feeds ONE bf16 dS to dK and dQ)."""
    return _attention_eval(qkv, lengths, B, S, NH, q, qoff, True)


def attention_delta_terms(dctx, ctx, B, S, NH, qoff=None):
    """(-sum(dO * O), sum |dO * O|) per (query, head) in float64, in the layout of PlbAttn.delta: [B, NH, S], or [NH, Nq]
    for compact queries."""
    n = B * S if qoff is None else int(qoff[-1])
    t = (dctx.double()[:n] * ctx.double()[:n]).reshape(n, NH, 64)
    ref, mag = -t.sum(-1), t.abs().sum(-1)
    if qoff is None:
        return tuple(v.reshape(B, S, NH).permute(0, 2, 1) for v in (ref, mag))
    return ref.T, mag.T


def check_delta(got, ref, mag, tol=1e-5):
    """|delta - ref| <= tol x sum |dO * O| per row: 64 fp32 products accumulated in fp32 are within 64 x 2^-24 = 4e-6 of
    the absolute sum."""
    err = (got.double() - ref).abs()
    bad = err > tol * mag
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"delta{list(i)}: got {float(got[i])!r}, want {float(ref[i])!r}: off by {float(err[i]):.3e} > "
                             f"{tol:g} x {float(mag[i]):.3e}; {int(bad.sum())} rows over")


def check_rows(name, got, ref, model, NH, valid=None, n_abs=0, factor=ROW_FACTOR):
    """The row contract for one output. got / ref / model [R, NH*64]: the kernel's rows, the float64 reference, the rounding
    model. valid [R] bool: rows outside it (padded keys / queries) must be exactly 0 in got. Of the valid (row, head)
    pairs, those whose reference norm is below ROW_TINY of the largest are held to |got| < ROW_ABS, and there must be
    exactly n_abs of them; every other pair is held to ||got - ref|| / ||ref|| <= factor x the model's worst such pair.
    Returns {"model": the model's maximum, "got": got's maximum, "bound", "n_abs"}; raises AssertionError naming the row."""
    R = ref.shape[0]
    g, f, mo = (t.double()[:R].reshape(R, NH, 64) for t in (got, ref, model))
    ok = torch.ones(R, dtype=torch.bool, device=ref.device) if valid is None else valid.to(ref.device)
    if not bool((g[~ok] == 0).all()):
        r = int((g[~ok] != 0).flatten(1).any(1).nonzero()[0])
        raise AssertionError(f"{name}: padded row {int((~ok).nonzero()[r])} is not exactly zero")
    den = f.norm(dim=-1)
    okh = ok[:, None].expand(R, NH)
    tiny = okh & (den < ROW_TINY * den[okh].max())
    rel = okh & ~tiny
    stats = {"model": 0.0, "got": 0.0, "bound": 0.0, "n_abs": int(tiny.sum())}
    if stats["n_abs"] != n_abs:
        raise AssertionError(f"{name}: {stats['n_abs']} (row, head) pairs fall under the absolute check, {n_abs} predicted")
    if n_abs:
        worst = g.abs().amax(-1).masked_fill(~tiny, 0.0)
        if float(worst.max()) >= ROW_ABS:
            r, h = divmod(int(worst.argmax()), NH)
            raise AssertionError(f"{name}: row {r} head {h} has a zero reference, got |x| up to {float(worst.max()):.3e}")
    if bool(rel.any()):
        eg = ((g - f).norm(dim=-1) / den.clamp_min(1e-300)).masked_fill(~rel, 0.0)
        em = ((mo - f).norm(dim=-1) / den.clamp_min(1e-300)).masked_fill(~rel, 0.0)
        stats.update(model=float(em.max()), got=float(eg.max()), bound=factor * float(em.max()))
        if not (torch.isfinite(eg).all() and stats["got"] <= stats["bound"]):
            eg = torch.nan_to_num(eg, nan=float("inf"))
            r, h = divmod(int(eg.argmax()), NH)
            raise AssertionError(f"{name}: row {r} head {h} is off by {float(eg[r, h]):.3e} of its norm; the bound is "
                                 f"{factor:g} x the rounding model's worst row {stats['model']:.3e} = {stats['bound']:.3e}; "
                                 f"{int((eg > stats['bound']).sum())} of {int(rel.sum())} rows over")
    return stats


# ---- call-history independence (tests/test_call_history_host.py) -----------------------------------------------------------
# A call on a used engine must leave the gradient buffer a fresh engine's call leaves, bit for bit. When two gradient buffers
# that should be the same are not, the report names the parameter tensors and the coordinates: that is the way back to the
# launch that summed a stale row.
def _bits(t):
    t = t.detach().reshape(-1)
    assert t.dtype == torch.float32, t.dtype
    return t.contiguous().view(torch.int32)


def first_difference(engine_like, a, b):
    """a, b: two flat fp32 buffers laid out as ``engine_like.layout`` says ({name: (offset, size, shape)}, as
    HipEngine.layout; the buffers may end before the layout does, e.g. grads[:trainable]). Returns [] when they are the
    same, else one record per differing tensor, in layout order: dict(name, count, index — the first differing element as
    a coordinate of the tensor's shape —, a, b — the two values there —, a_bits, b_bits). Elements no tensor of the layout
    covers are reported under the name "(outside the layout)" with a flat index.

    "The same" is equality of BIT PATTERNS, with one exception: a NaN equals a NaN of identical bits (a float == would call
    them different), a NaN differs from any number and from a NaN of other bits, 1.0 differs from its neighbour. The
    exception: -0.0 and +0.0 are equal, as for torch.equal — an fp32 sum that started at +0 and added -0, or a product of
    an exact zero with a stale value of either sign, is not a leak."""
    ia, ib = _bits(a), _bits(b)
    if ia.shape != ib.shape:
        raise ValueError(f"buffers of {ia.numel()} and {ib.numel()} elements")
    diff = (ia != ib) & (((ia | ib) & 0x7FFFFFFF) != 0)
    if not bool(diff.any()):
        return []
    n = ia.numel()
    covered = torch.zeros(n, dtype=torch.bool, device=diff.device)
    out = []

    def record(name, d, base, shape):
        flat = int(d.nonzero()[0])
        i = base + flat
        coord = [] if shape else [flat]
        for dim in reversed(shape or ()):   # needs only the shape: also given for a tensor that the buffer ends inside
            flat, c = divmod(flat, dim)
            coord.insert(0, c)
        out.append(dict(name=name, count=int(d.sum()), index=[int(c) for c in coord],
                        a=float(a.reshape(-1)[i]), b=float(b.reshape(-1)[i]),
                        a_bits=int(ia[i]) & 0xFFFFFFFF, b_bits=int(ib[i]) & 0xFFFFFFFF))

    for name, (off, size, shape) in engine_like.layout.items():
        lo, hi = min(off, n), min(off + size, n)
        if hi <= lo:
            continue
        covered[lo:hi] = True
        d = diff[lo:hi]
        if bool(d.any()):
            record(name, d, lo, tuple(shape))
    rest = diff & ~covered
    if bool(rest.any()):
        record("(outside the layout)", rest, 0, None)
    return out


def format_difference(records):
    return "; ".join(f"{r['name']}: {r['count']} element{'s' * (r['count'] != 1)}, first at {r['index']}: "
                     f"{r['a']!r} (0x{r['a_bits']:08x}) vs {r['b']!r} (0x{r['b_bits']:08x})" for r in records)


def assert_same_bits(engine_like, a, b, what):
    """Raises AssertionError with first_difference's report, e.g. "gradients after H1: ...value.weight: 31 elements, first
    at [17, 203]: 1.5 (0x3fc00000) vs 1.25 (0x3fa00000)"."""
    rec = first_difference(engine_like, a, b)
    if rec:
        raise AssertionError(f"{what}: {len(rec)} tensor{'s' * (len(rec) != 1)} differ — {format_difference(rec)}")


# ---- exact arithmetic for the GEMM family (tests/test_gpu_gemm_exact.py, tests/test_gemm_exact_host.py) -------------------
# With small-integer operands every product and every partial sum of a GEMM is an exact fp32 number as long as the sum of
# the terms' magnitudes stays below 2^24 (times the power-of-two unit the operands are multiples of): the result no longer
# depends on summation order, tile form, K-loop form or split count. fp32 outputs must then EQUAL the float64 reference
# and bf16 outputs its round-to-nearest-even; a dropped, duplicated or misplaced contribution changes bits.
EXACT_LIMIT = 2.0 ** 24
SENTINEL = 0.33      # not a multiple of any unit used here, in bf16 (0.330078125) or fp32: no exact result can equal it
_F8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}

# The case tables. form -> (TM, TN, (M, N) with 9 workgroups in flight, K-tile counts of 64 elements)
BIG_KTILES = (1, 2, 3, 4, 5, 6, 7, 10, 11, 13, 33)   # prologue, every drain length, the 10-slot ring's wraps (5 / 10) + 1, long
NT_FORMS = {128: (128, 128, (384, 384), (1, 2, 3, 7)), 256: (256, 256, (768, 768), BIG_KTILES),
            384: (128, 384, (384, 1152), BIG_KTILES), 1256: (128, 256, (384, 768), BIG_KTILES)}
NT_FORM_PARAMS = [(128, -1), (256, 0), (256, 1), (384, 0), (384, 1), (1256, 0), (1256, 1)]   # (form, K-loop form)
NT_TAILS = ((128, 4), (128, 124), (256, 188), (128, 260))        # the 128 kernel's column tails (M, N)
NT_STRIDE_KTILES = 3
FP8_NT_FORMS = {384: (128, 384, (384, 1152)), 1256: (128, 256, (1152, 256))}   # the tiles plb_launch_gemm_nt_fp8 picks
FP8_KTILES = (1, 2, 3, 4, 5, 11)                                  # of 128 elements
FP8_DEQ = (2.0 ** -3, 2.0 ** -2)
LN_CASES = ((1024, 768, 64), (1024, 768, 192), (1024, 1024, 128))
CE_SHAPE, CE_COLS, CE_TILES = (256, 512, 192), (200, 300, 512), (256, 1256)
GELU_KTILES = 2      # K = 128: with B x 2^-4 the pre-activation has a standard deviation of about 4.7
GELU_UNIT = 2.0 ** -4
# (Mtot, Ncols, N, K, splits, rows_per_split, lda, ldb)
TN_SMALL = ((64, 128, 128, 128, 1, 64, 128, 128), (192, 256, 188, 136, 1, 192, 264, 136),
            (320, 128, 128, 64, 3, 128, 128, 64),      # the last split is short
            (128, 256, 256, 256, 3, 64, 256, 256))     # the third split is empty
# the big kernel: rows_per_split 64 x {1..5} with 2 splits over Ncols, K in {256, 512}; short and empty last split; N < Ncols;
# splits == 1 is the direct form (the kernel writes the output itself)
TN_BIG = tuple((mt, nc, n, k, sp, rps, nc + 8, k + 8) for mt, nc, n, k, sp, rps in (
    (128, 256, 256, 256, 2, 64), (256, 512, 512, 256, 2, 128), (384, 256, 256, 512, 2, 192), (512, 512, 512, 512, 2, 256),
    (640, 256, 256, 256, 2, 320), (320, 256, 256, 512, 2, 192), (128, 512, 512, 256, 2, 128), (256, 256, 188, 256, 2, 128),
    (192, 256, 256, 256, 1, 192), (320, 512, 188, 512, 1, 320)))
# the fp8 kernel: rows_per_split 128 x {1..5}; strides in bytes
TN_FP8 = tuple((mt, nc, nc, k, sp, rps, nc + 16, k + 32) for mt, nc, k, sp, rps in (
    (256, 256, 256, 2, 128), (512, 512, 256, 2, 256), (768, 256, 512, 2, 384), (1024, 512, 512, 2, 512),
    (1280, 256, 256, 2, 640), (384, 256, 512, 2, 256), (256, 512, 256, 2, 256), (384, 256, 256, 1, 384)))
# (kind, Mtot, Ncols, N, K, lda, ldb): splits and rows_per_split are the PLAN's (csrc/gemm_tn_plan.h), not a table's. 8192 rows
# is the smallest call the plan sends to the pipeline kernels: 128 splits of 64 rows in bf16, 64 of 128 in fp8, so every
# split runs the one-K-tile path; the small kernel with N < Ncols (the phoneme head's form): 6 splits of 64 rows
TN_PLANNED = (("big", 8192, 256, 256, 256, 264, 264), ("fp8", 8192, 256, 256, 256, 272, 288), ("small", 384, 256, 188, 136, 264, 136))
TN_PLANNED_SPLITS = ((128, 64), (64, 128), (6, 64))


def int_operands(shape, lo, hi, seed, kind="bf16", unit=1.0):
    """Integers in [lo, hi] x unit (a power of two), generated on the CPU: kind "bf16" / "f32" -> a tensor of that type,
    "e4m3" / "e5m2" -> the 1-byte image (uint8)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(lo, hi + 1, tuple(shape), generator=g).float() * unit
    if kind == "f32":
        return x
    return x.to(torch.bfloat16) if kind == "bf16" else x.to(_F8[kind]).view(torch.uint8)


def int_bias(n, seed, hi=64, unit=1.0):
    return int_operands((n,), -hi, hi, seed, "f32", unit)


def int_residual(M, N, seed, hi=128):
    return int_operands((M, N), -hi, hi, seed, "bf16")


def operand_values(x, kind="bf16"):
    """The values an operand holds, as float64 (a 1-byte image decoded)."""
    return x.view(_F8[kind]).float().double() if kind in _F8 else x.double()


def exact_bound(A, B, bias=None, res=None, unit=1.0):
    """max(|A|.|B|^T + |bias| + |res|) in float64, in units of `unit` (the power of two every term is a multiple of). Below
    2^24 every partial sum, in any order, is an exact fp32 number. A condition, not a tolerance. A [M,K], B [N,K] values."""
    s = A.double().abs() @ B.double().abs().T
    if bias is not None:
        s = s + bias.double().abs()
    if res is not None:
        s = s + res.double().abs()
    return float(s.max()) / unit


def exact_nt(A, B, bias=None, res=None, scale=1.0):
    """(A.B^T) x scale + bias + res in float64: exact under exact_bound."""
    s = (A.double() @ B.double().T) * scale
    if bias is not None:
        s = s + bias.double()
    if res is not None:
        s = s + res.double()
    return s


def rne_bf16(ref):
    """The bf16 expectation of an exact float64 result: it fits fp32 exactly, torch's cast rounds to nearest even."""
    return ref.float().to(torch.bfloat16)


def first_mismatch(got, want, TM, TN):
    """None when got == want element for element (value equality, as torch.equal: the sign of zero is not part of the
    contract); else the report used as the assertion message: how many elements differ, the first (row, col), its row
    tile, column tile and 64x32 wave patch inside the tile, and the two values there."""
    g, w = got.double(), want.double()
    assert g.shape == w.shape, (tuple(g.shape), tuple(w.shape))
    bad = g != w
    if not bool(bad.any()):
        return None
    r, c = (int(v) for v in bad.nonzero()[0])
    return (f"{int(bad.sum())} of {bad.numel()} elements differ; first at ({r}, {c}) = row tile {r // TM}, column tile "
            f"{c // TN}, wave patch ({r % TM // 64}, {c % TN // 32}): got {float(g[r, c])!r}, want {float(w[r, c])!r}")


def mismatch_location(got, want, TM, TN):
    """(count, row tile, column tile, (patch row, patch column)) of first_mismatch's report, or None."""
    bad = got.double() != want.double()
    if not bool(bad.any()):
        return None
    r, c = (int(v) for v in bad.nonzero()[0])
    return int(bad.sum()), r // TM, c // TN, (r % TM // 64, c % TN // 32)


def assert_exact(got, want, TM, TN, what):
    msg = first_mismatch(got, want, TM, TN)
    assert msg is None, f"{what}: {msg}"


def assert_untouched(t, what):
    """Every element still holds SENTINEL (as rounded to t's type)."""
    s = torch.tensor(SENTINEL, dtype=t.dtype)
    n = int((t != s.to(t.device)).sum())
    assert n == 0, f"{what}: {n} elements that must not be written were"


def spacing_bf16(x):
    """The distance between neighbouring bf16 numbers at |x| (float64 in, float64 out; at 0: the smallest normal's)."""
    a = x.double().abs().clamp_min(2.0 ** -126).contiguous()
    return (a.view(torch.int64) & 0x7FF0000000000000).view(torch.float64) * 2.0 ** -7    # 2^floor(log2 |x|) x 2^-7, exactly


_K0, _K1 = 0.7978845608028654, 0.044715


def gelu64(x):
    """gelu_new in float64 in the cancellation-free form x / (1 + exp(-2z)): 0.5 x (1 + tanh z) returns 0 below x = -7.2."""
    x = x.double()
    return x / (1.0 + torch.exp(-2.0 * _K0 * (x + _K1 * x ** 3)))


def gelu_grad64(x):
    x = x.double()
    s = 1.0 / (1.0 + torch.exp(-2.0 * _K0 * (x + _K1 * x ** 3)))
    return s + x * s * (1.0 - s) * 2.0 * _K0 * (1.0 + 3.0 * _K1 * x * x)


def _fma32(a, b, c):
    import numpy as np
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gelu_f32_restatement(x):
    """csrc/common.h gelu_new_f / gelu_new_grad_f restated in float32 numpy, same operation order and constants (exp2 and
    the reciprocal by numpy instead of v_exp_f32 / v_rcp_f32). x: float32 array -> (gelu, gelu')."""
    import numpy as np
    f = np.float32
    x = x.astype(f)
    x2 = x * x
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp2(x * _fma32(x2, np.full_like(x, f(-0.10294324)), np.full_like(x, f(-2.3022082)))).astype(f)
        s = (f(1.0) / (f(1.0) + e)).astype(f)
    w = x * _fma32(x2, np.full_like(x, f(0.21406444)), np.full_like(x, f(1.5957691)))
    return x * s, _fma32(s, w * (f(1.0) - s), s)


class Ln:
    """Buffers of one fused GEMM + LayerNorm launch (tests/test_gpu_gemm_ln.py, tests/test_gpu_gemm_exact.py)."""

    def __init__(self, M, N, K, seed=0, dev="cuda"):
        def randbf(*shape, scale=1.0, seed=0):
            g = torch.Generator(device="cpu").manual_seed(seed)
            return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)

        self.M, self.N, self.K = M, N, K
        self.A, self.B = randbf(M, K, seed=seed + 1), randbf(N, K, scale=K ** -0.5, seed=seed + 2)
        self.bias = torch.randn(N, generator=torch.Generator().manual_seed(seed + 3)).to(dev)
        self.res = randbf(M, N, seed=seed + 4)
        g = torch.Generator().manual_seed(seed + 5)
        self.gamma = (1.0 + 0.3 * torch.randn(N, generator=g)).to(dev)
        self.beta = (0.2 * torch.randn(N, generator=g)).to(dev)
        nbn = N // (384 if N % 384 == 0 else 256)
        self.nbn = nbn
        self.xchg = torch.zeros(M // 128 * nbn * nbn * 128 * 2, dtype=torch.int64, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.mean = torch.zeros(M, dtype=torch.float32, device=dev)
        self.rstd = torch.zeros(M, dtype=torch.float32, device=dev)

    def params(self):
        p = _lib.PlbGemmNT()
        p.A, p.lda, p.B, p.ldb = self.A.data_ptr(), self.K, self.B.data_ptr(), self.K
        p.M, p.N, p.K, p.Mstore = self.M, self.N, self.K, self.M
        p.ln_gamma, p.ln_beta, p.ln_mean, p.ln_rstd = self.gamma.data_ptr(), self.beta.data_ptr(), self.mean.data_ptr(), self.rstd.data_ptr()
        p.ln_eps = 1e-12
        p.ln_xchg, p.ln_err = self.xchg.data_ptr(), self.err.data_ptr()
        return p


def gemm_nt_fp8(A8, B8, N, deq, bias=None, res=None, a_bf8=0, C=None, fill=None):
    """plb_launch_gemm_nt_fp8, act 0: A8 [M,K] / B8 [N,K] 1-byte images (uint8), deq = (1 / scale of A, of B) -> bf16
    C [M,N] = (A.B^T) x deq_a x deq_b + bias + res. C: a caller-provided output (the in-place case)."""
    L = _lib.lib()
    M, K = A8.shape
    d = torch.tensor(list(deq), dtype=torch.float32, device=A8.device)
    Cb = C if C is not None else _out(M, N, torch.bfloat16, A8.device, fill)
    p = _lib.PlbGemmNT()
    p.A, p.lda, p.B, p.ldb = A8.data_ptr(), A8.stride(0), B8.data_ptr(), B8.stride(0)
    p.M, p.N, p.K, p.Mstore = M, N, K, M
    p.deq_a, p.deq_b = d.data_ptr(), d.data_ptr() + 4
    p.bias = bias.data_ptr() if bias is not None else None
    if res is not None:
        p.res, p.ldr = res.data_ptr(), res.stride(0)
    p.C, p.ldc = Cb.data_ptr(), Cb.stride(0)
    rc = L.plb_launch_gemm_nt_fp8(_byref(p), 0, int(a_bf8), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return Cb


def gemm_tn_slabs(A, B, N, splits, rows_per_split, kind="small", deq=None, tail=0):
    """The weight-gradient kernels without the reduction. A [Mtot, Ncols], B [Mtot, K]: bf16, or (kind "fp8") the e5m2 and
    e4m3 images as uint8; row strides are the tensors' (bytes for the images). Returns the SENTINEL-filled flat fp32 buffer
    the launch wrote its [splits][N][K] slabs into, with `tail` more floats behind them that must stay untouched."""
    L = _lib.lib()
    Mtot, Ncols = A.shape
    K = B.shape[1]
    buf = torch.full((splits * N * K + tail,), SENTINEL, dtype=torch.float32, device=A.device)
    p = _lib.PlbGemmTN()
    p.A, p.lda, p.Ncols, p.B, p.ldb = A.data_ptr(), A.stride(0), Ncols, B.data_ptr(), B.stride(0)
    p.Mtot, p.N, p.K, p.rows_per_split, p.splits, p.slab = Mtot, N, K, rows_per_split, splits, buf.data_ptr()
    if kind == "fp8":
        d = torch.tensor(list(deq), dtype=torch.float32, device=A.device)
        p.deq_a, p.deq_b = d.data_ptr(), d.data_ptr() + 4
    fn = {"small": L.plb_launch_gemm_tn, "big": L.plb_launch_gemm_tn_big, "fp8": L.plb_launch_gemm_tn_fp8}[kind]
    rc = fn(_byref(p), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return buf


def reduce_slabs(slab, splits, n, out, accumulate):
    rc = _lib.lib().plb_launch_reduce_slabs(slab.data_ptr(), splits, n, out.data_ptr(), int(accumulate), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def split_rows(Mtot, splits, rows_per_split):
    """[(first row, end row)] of every split: the last may be short or empty."""
    return [(min(s * rows_per_split, Mtot), min((s + 1) * rows_per_split, Mtot)) for s in range(splits)]


def exact_tn(A, B, N, splits, rows_per_split, scale=1.0):
    """float64 [splits][N][K]: slab s = A[rows of s, :N]^T . B[rows of s] x scale."""
    A, B = A.double(), B.double()
    return torch.stack([A[a:b, :N].T @ B[a:b] * scale for a, b in split_rows(A.shape[0], splits, rows_per_split)])


def nt_operands(M, N, K, seed, kinds=("bf16", "bf16"), b_unit=1.0, brows=None, bias_hi=64):
    """The operands of one exact NT case, on the CPU: A [M,K] and B [brows or N, K] in [-4, 4] (B x b_unit), integer bias
    in [-bias_hi, bias_hi], integer bf16 residual in [-128, 128]."""
    A = int_operands((M, K), -4, 4, seed, kinds[0])
    B = int_operands((brows or N, K), -4, 4, seed + 1, kinds[1], b_unit)
    return A, B, int_bias(N, seed + 2, bias_hi), int_residual(M, N, seed + 3)


def tn_operands(Mtot, Ncols, K, seed, kinds=("bf16", "bf16")):
    return int_operands((Mtot, Ncols), -4, 4, seed, kinds[0]), int_operands((Mtot, K), -4, 4, seed + 1, kinds[1])


def exact_cases():
    """Every (name, A values, B values, bias, res, unit) the GPU module launches, built as it builds them — for the premise
    check of tests/test_gemm_exact_host.py. NT: A [M,K], B [N,K]; TN rows come transposed (A^T, B^T: the sum runs over rows)."""
    for form, (TM, TN, (M, N), kts) in NT_FORMS.items():
        for kt in kts:
            A, B, bias, res = nt_operands(M, N, 64 * kt, 1000 * form + kt)
            yield f"nt {form} kt {kt}", A, B, bias, res, 1.0
        A, B, bias, res = nt_operands(M, N, 64 * GELU_KTILES, 7000 + form, b_unit=GELU_UNIT, bias_hi=2)
        yield f"gelu {form}", A, B, bias, None, GELU_UNIT
    for M, N in NT_TAILS:
        for kt in NT_FORMS[128][3]:
            A, B, bias, res = nt_operands(M, N, 64 * kt, 2000 + N + kt, brows=(N + 127) // 128 * 128)
            yield f"tail {M}x{N} kt {kt}", A, B[:N], bias, res, 1.0
    unit8 = FP8_DEQ[0] * FP8_DEQ[1]
    for form, (TM, TN, (M, N)) in FP8_NT_FORMS.items():
        for bf8 in (0, 1):
            for kt in FP8_KTILES:
                A, B, bias, res = nt_operands(M, N, 128 * kt, 3000 + form + 10 * kt + bf8, kinds=("e5m2" if bf8 else "e4m3", "e4m3"))
                yield (f"fp8 nt {form} bf8 {bf8} kt {kt}", operand_values(A, "e5m2" if bf8 else "e4m3") * FP8_DEQ[0],
                       operand_values(B, "e4m3") * FP8_DEQ[1], bias, res, unit8)
    for M, N, K in LN_CASES:
        A, B, bias, res = nt_operands(M, N, K, 4000 + N + K)
        yield f"ln {M}x{N}x{K}", A, B, bias, res, 1.0
    M, N, K = CE_SHAPE
    A, B, bias, _ = nt_operands(M, N, K, 5000)
    yield "ce", A, B, bias, None, 1.0
    for i, (Mtot, Ncols, N, K, splits, rps, lda, ldb) in enumerate(TN_SMALL + TN_BIG):
        A, B = tn_operands(Mtot, Ncols, K, 6000 + i)
        yield f"tn {i}", A.T, B.T, None, None, 1.0
    for i, (Mtot, Ncols, N, K, splits, rps, lda, ldb) in enumerate(TN_FP8):
        A, B = tn_operands(Mtot, Ncols, K, 6500 + i, kinds=("e5m2", "e4m3"))
        yield f"tn fp8 {i}", operand_values(A, "e5m2").T * FP8_DEQ[0], operand_values(B, "e4m3").T * FP8_DEQ[1], None, None, unit8
    for i, (kind, Mtot, Ncols, N, K, lda, ldb) in enumerate(TN_PLANNED):
        if kind == "fp8":
            A, B = tn_operands(Mtot, Ncols, K, 6600 + i, kinds=("e5m2", "e4m3"))
            yield f"tn planned {i}", operand_values(A, "e5m2").T * FP8_DEQ[0], operand_values(B, "e4m3").T * FP8_DEQ[1], None, None, unit8
        else:
            A, B = tn_operands(Mtot, Ncols, K, 6600 + i)
            yield f"tn planned {i}", A.T, B.T, None, None, 1.0


# ---- the LayerNorm element contract (tests/test_gpu_layernorm_rows.py, tests/test_layernorm_rows_host.py) -----------------
# Every element a LayerNorm kernel stores — the four standalone kernels of csrc/layernorm.hip and forms 5 / 6 of the NT pipeline
# GEMM, bf16 and fp8 — is held to the float64 evaluation of the same stored inputs:
#     |got - ref| <= 0.5 x spacing_bf16(ref) + delta x cond
# one round-to-nearest of the exact value plus the fp32 arithmetic behind it, weighted by the element's condition term.
# Nothing below calls a kernel or reads a kernel's output to form a bound.
LN_EPS = 1e-12
DELTA0 = 2.0 ** -18        # <= 32 fp32 roundings stand behind any sum of these kernels (<= 24 sequential per lane, then the
                           # trees): 32 x 2^-24 = 2^-19, and a factor 2
LN_STAT_FLOOR = 2.0 ** -20  # 8 fp32 ulps: rsqrtf and the final multiply
LN_CLASSES = ("plain", "off4", "off16", "small", "eps", "large", "spike", "zero", "nearconst")
LN_BWD_CLASSES = ("plain", "off4", "off16", "small", "large", "spike")
LN_NEARCONST_SEED = 0      # ln_rows(1024, 768, seed, ("nearconst",)) holds a row whose merged M2 is <= 0 in the tile
                           # restatement (tests/test_layernorm_rows_host.py searches and pins it)


def ln_rows(T, W, seed, classes=LN_CLASSES):
    """bf16 rows [T, W] on the CPU, row r in class classes[r % len(classes)], and the class index per row. Classes: plain
    N(0,1); off4 N(4,1); off16 N(16,1); small N(0,1) x 2^-12; eps N(0,1) x 2^-20 (variance ~ eps = 1e-12); large N(0,1) x
    2^10; spike N(0,1) with one element 200 at column (r * 37) % W; zero; nearconst: a bf16 constant in [1, 60] that
    varies with r, 1-3 elements one bf16 step up."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, W, generator=g)
    u = torch.rand(T, 5, generator=g)
    r = torch.arange(T)
    cls = r % len(classes)
    near = None
    for k, name in enumerate(classes):
        rows = (cls == k).nonzero().flatten()
        if name == "plain":
            pass
        elif name in ("off4", "off16"):
            x[rows] += float(name[3:])
        elif name in ("small", "eps", "large"):
            x[rows] *= {"small": 2.0 ** -12, "eps": 2.0 ** -20, "large": 2.0 ** 10}[name]
        elif name == "spike":
            x[rows, (rows * 37) % W] = 200.0
        elif name == "zero":
            x[rows] = 0.0
        elif name == "nearconst":
            near = rows
        else:
            raise ValueError(name)
    xb = x.to(torch.bfloat16)
    if near is not None and near.numel():
        c = (1.0 + 59.0 * u[near, 0]).to(torch.bfloat16)
        up = (c.view(torch.int16) + 1).view(torch.bfloat16)          # positive: the next bf16 up
        xb[near] = c[:, None]
        n = 1 + (u[near, 1] * 3).long().clamp(max=2)
        cols = (u[near, 2:5] * W).long().clamp(max=W - 1)
        for j in range(3):
            sel = n > j
            xb[near[sel], cols[sel, j]] = up[sel]
    return xb, cls


def layernorm_fp64(x, gamma, beta, eps=LN_EPS):
    """(mean [T], rstd [T], xhat [T,H], y [T,H]) in float64 from the input as stored; biased variance, eps inside the root;
    y is not rounded."""
    x = x.double()
    mean = x.mean(1)
    d = x - mean[:, None]
    rstd = ((d * d).mean(1) + eps) ** -0.5
    xhat = d * rstd[:, None]
    return mean, rstd, xhat, xhat * gamma.double() + beta.double()


def ln_fwd_cond(xhat, gamma, beta, mean, rstd):
    """|gamma_j| (1 + |xhat_ij| + |mu_i| rstd_i) + |beta_j|: what an fp32 rounding of the statistics or of the products moves
    y by. The |mu| rstd term is the mean's own fp32 rounding (2^-24 |mu|, whatever the summation) seen through x - mean: it
    is what conditions a near-constant row (sigma << |mu|), and on a centred row it adds nothing
    (tests/test_layernorm_rows_host.py: without it honest fp32 arithmetic fails the nearconst class)."""
    return gamma.double().abs() * (1.0 + xhat.abs() + (mean.abs() * rstd)[:, None]) + beta.double().abs()


class LnBwd:
    """layernorm_bwd_fp64's results: dx (unrounded), dgamma, dbeta, the magnitude sums per column and the condition term."""
    __slots__ = ("dx", "dgamma", "dbeta", "mag_gamma", "mag_beta", "cond", "xhat")


def layernorm_bwd_fp64(x, mean, rstd, gamma, dy):
    """LayerNorm backward in float64 from x, dy as stored and the SUPPLIED fp32 mean / rstd (the backward kernels' contract:
    they never recompute statistics). dx = rstd (g - mean_j g - xhat mean_j(g xhat)), g = dy gamma; dgamma = sum_i dy xhat,
    dbeta = sum_i dy with sum |dy xhat|, sum |dy|; cond = rstd (|g| + mean_j |g| + |xhat| mean_j |g xhat|)."""
    x, dy, rs = x.double(), dy.double(), rstd.double()[:, None]
    xhat = (x - mean.double()[:, None]) * rs
    g = dy * gamma.double()
    o = LnBwd()
    o.xhat = xhat
    o.dx = rs * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    t = dy * xhat
    o.dgamma, o.dbeta, o.mag_gamma, o.mag_beta = t.sum(0), dy.sum(0), t.abs().sum(0), dy.abs().sum(0)
    o.cond = rs * (g.abs() + g.abs().mean(1, keepdim=True) + xhat.abs() * (g * xhat).abs().mean(1, keepdim=True))
    return o


def _np32(t):
    return t.detach().cpu().float().numpy()


def _tree(a):
    """Pairwise fp32 sum over the last axis (a power of two): the butterfly of a wave reduction."""
    while a.shape[-1] > 1:
        h = a.shape[-1] // 2
        a = a[..., :h] + a[..., h:]
    return a[..., 0]


def lane_tree_sum(v):
    """fp32 sum over the last axis as the standalone kernels form it: 64 lanes each add their <= 16 values one after the
    other, then a 6-level tree. v: float32 numpy [T, H], H <= 1024."""
    import numpy as np
    T, H = v.shape
    L = -(-H // 64)
    pad = np.zeros((T, L * 64), np.float32)
    pad[:, :H] = v
    pad = pad.reshape(T, L, 64)
    s = np.zeros((T, 64), np.float32)
    for i in range(L):
        s = s + pad[:, i]
    return _tree(s)


def _two_pass(v, eps):
    import numpy as np
    f = np.float32
    H = v.shape[1]
    inv = f(1.0) / f(H)
    mean = lane_tree_sum(v) * inv
    d = v - mean[:, None]
    var = lane_tree_sum(d * d) * inv
    return mean, f(1.0) / np.sqrt(var + f(eps)), var * f(H)


def _tile_stats(v, TN, eps, contract=True):
    """Form 5 (csrc/gemm_nt_pipeline.h): per lane s1 / s2 over its 4-column groups in order, xor 16 / 32 across the four
    lanes that share a row, the four wn partials, (mean, M2) of the tile in one pass, the merge across tiles. contract: the
    tile's pb - pa * mt as one fused multiply-add (what the compiler is free to emit) or as two rounded operations."""
    import numpy as np
    f = np.float32
    T, N = v.shape
    nbn, nbh = N // TN, TN // 128
    # column inside a tile = nh * 128 + wn * 32 + ni * 16 + fq * 4 + r  ->  [T, tile, wn, fq, (nh, ni), r]
    t = v.reshape(T, nbn, nbh, 4, 2, 4, 4).transpose(0, 1, 3, 5, 2, 4, 6).reshape(T, nbn, 4, 4, nbh * 2, 4)
    s1 = np.zeros((T, nbn, 4, 4), f)
    s2 = np.zeros((T, nbn, 4, 4), f)
    for gI in range(nbh * 2):
        a, b, c, d = (t[..., gI, j] for j in range(4))
        s1 = s1 + ((a + b) + (c + d))
        s2 = s2 + ((a * a + b * b) + (c * c + d * d))
    fold = lambda s: (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])   # noqa: E731
    pa, pb = fold(fold(s1)), fold(fold(s2))
    mt = pa * (f(1.0) / f(TN))
    pb = _fma32(-pa, mt, pb) if contract else pb - pa * mt
    mean = np.zeros(T, f)
    for j in range(nbn):
        mean = mean + mt[:, j]
    mean = mean * (f(1.0) / f(nbn))
    m2 = np.zeros(T, f)
    for j in range(nbn):
        m2 = m2 + (pb[:, j] + f(TN) * (mt[:, j] - mean) * (mt[:, j] - mean))
    rstd = f(1.0) / np.sqrt(np.maximum(m2, f(0.0)) * (f(1.0) / f(N)) + f(eps))
    return mean, rstd, m2


class LnStats:
    """layernorm_stats_f32's results, per row: rstd_err, mean_err (worst over the orders), m2 (smallest over the orders: the
    fp32 sum of squared deviations before the clamp), and mean / rstd of order 0 (the kernels' own column order)."""
    __slots__ = ("rstd_err", "mean_err", "m2", "mean", "rstd")


def layernorm_stats_f32(x, form, orders=8, eps=LN_EPS):
    """A numpy float32 restatement of the statistics only. form "two_pass": the standalone kernels (lane_tree_sum, the mean
    subtracted before squaring); form ("tile", TN): form 5 of the pipeline GEMM (_tile_stats). Evaluated over `orders`
    summation orders (order 0: the columns as they are; the others: shuffled, inside a tile for the tile form; the tile form
    each time with and without the contraction of pb - pa * mt) -> the worst
    relative rstd error and the worst |mean - mu| / (|mu| + sigma) per row against float64. Reads no kernel output."""
    import numpy as np
    v = _np32(x)
    T, H = v.shape
    v64 = v.astype(np.float64)
    mu = v64.mean(1)
    var = ((v64 - mu[:, None]) ** 2).mean(1)
    rs = (var + eps) ** -0.5
    o = LnStats()
    o.rstd_err, o.mean_err, o.m2 = np.zeros(T), np.zeros(T), np.full(T, np.inf)
    rng = np.random.default_rng(H)
    for k in range(orders):
        w = v
        if k:
            if form == "two_pass":
                w = v[:, rng.permutation(H)]
            else:
                TN = form[1]
                w = v.reshape(T, H // TN, TN)[:, :, rng.permutation(TN)].reshape(T, H)
        w = np.ascontiguousarray(w)
        evals = [_two_pass(w, eps)] if form == "two_pass" else [_tile_stats(w, form[1], eps, c) for c in (True, False)]
        if k == 0:
            o.mean, o.rstd = evals[0][0], evals[0][1]
        for mean, rstd, m2 in evals:
            o.rstd_err = np.maximum(o.rstd_err, np.abs(rstd.astype(np.float64) / rs - 1.0))
            o.mean_err = np.maximum(o.mean_err, np.abs(mean.astype(np.float64) - mu) / (np.abs(mu) + np.sqrt(var) + 1e-300))
            o.m2 = np.minimum(o.m2, m2.astype(np.float64))
    return o


def ln_class_worst(per_row, cls, classes):
    """{class: the worst of a per-row figure over the rows of the class}."""
    import numpy as np
    c = cls.cpu().numpy()
    a = np.asarray(per_row, dtype=np.float64)
    return {name: float(a[c == k].max()) for k, name in enumerate(classes) if bool((c == k).any())}


def ln_row_bound(worst, cls, classes, floor, dev="cpu"):
    """Per row: max(floor, ROW_FACTOR x its class's worst restated figure) — the statistics' bound (floor LN_STAT_FLOOR) and
    the delta of the fused forward forms (floor DELTA0)."""
    per = torch.tensor([max(floor, ROW_FACTOR * worst.get(name, 0.0)) for name in classes], dtype=torch.float64)
    return per[cls.cpu()].to(dev)


def check_ln_elements(name, got, ref, cond, delta, cls=None, classes=LN_CLASSES):
    """Every element: |got - ref| <= 0.5 x spacing_bf16(ref) + delta_row x cond. got [T,H] as stored, ref / cond float64,
    delta a number or a float64 tensor [T]; cls [T]: the class index per row (for the report). Raises naming row, column,
    class, got, want and the count of elements over. Returns {class: the worst share of the fp32 allowance in use,
    max(0, err - 0.5 spacing) / (delta x cond)}: err / bound itself sits next to 1 on every element that falls near a
    rounding tie, whatever the arithmetic, so the share of the arithmetic term is what tells a tight kernel from a loose
    one. 0 where the element is within its rounding term (also where cond = 0: an exact zero)."""
    g = got.double()
    assert g.shape == ref.shape == cond.shape, (tuple(g.shape), tuple(ref.shape), tuple(cond.shape))
    T = g.shape[0]
    d = delta.to(ref.device).double()[:, None] if torch.is_tensor(delta) else float(delta)
    half = 0.5 * spacing_bf16(ref)
    arith = d * cond
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    cl = (torch.zeros(T, dtype=torch.long) if cls is None else cls).to(ref.device)
    bad = err > half + arith
    if bool(bad.any()):
        r, c = (int(v) for v in bad.nonzero()[0])
        cname = classes[int(cl[r])] if cls is not None else "-"
        raise AssertionError(f"{name}: element ({r}, {c}) of class {cname}: got {float(g[r, c])!r}, want {float(ref[r, c])!r}: "
                             f"off by {float(err[r, c]):.3e} > 0.5 x {float(2 * half[r, c]):.3e} + {float(arith[r, c]):.3e}; "
                             f"{int(bad.sum())} of {bad.numel()} elements over")
    over = (err - half).clamp_min(0.0)
    share = torch.where(over > 0, over / arith.clamp_min(1e-300), torch.zeros_like(over)).amax(1) if g.shape[1] else over.sum(1)
    return {classes[k] if cls is not None else "-": float(share[cl == k].max()) for k in cl.unique().tolist()}


def check_ln_stats(name, mean, rstd, x, bound_mean, bound_rstd, cls=None, classes=LN_CLASSES, eps=LN_EPS):
    """Per row: |rstd / rstd_ref - 1| <= bound_rstd and |mean - mu| / (|mu| + sigma) <= bound_mean (numbers or [T] tensors)
    against float64 statistics of x as stored. An all-zero row: mean == 0 exactly. Returns the (mean, rstd) figures per row."""
    x = x.double()
    mu = x.mean(1)
    var = ((x - mu[:, None]) ** 2).mean(1)
    rs = (var + eps) ** -0.5
    m, s = mean.double().to(x.device), rstd.double().to(x.device)
    em = (m - mu).abs() / (mu.abs() + var.sqrt()).clamp_min(1e-300)
    em = torch.where(m == mu, torch.zeros_like(em), em)          # an exact mean (a zero row: 0 / 0)
    es = (s / rs - 1.0).abs()
    as_rows = lambda b: b.to(x.device).double() if torch.is_tensor(b) else torch.full_like(em, float(b))   # noqa: E731
    for what, e, b, gv, rv in (("mean", em, as_rows(bound_mean), m, mu), ("rstd", es, as_rows(bound_rstd), s, rs)):
        bad = ~(torch.isfinite(gv) & (e <= b))
        if bool(bad.any()):
            r = int(bad.nonzero()[0])
            cname = classes[int(cls[r])] if cls is not None else "-"
            raise AssertionError(f"{name}: {what} of row {r} (class {cname}): got {float(gv[r])!r}, want {float(rv[r])!r}: off by "
                                 f"{float(e[r]):.3e} > {float(b[r]):.3e}; {int(bad.sum())} rows over")
    zero = (x == 0).all(1)
    if bool(zero.any()):
        assert bool((m[zero] == 0).all()), f"{name}: the mean of an all-zero row is not exactly 0"
    return em, es


def check_ln_partials(name, got, ref, mag, rows_per_lane):
    """A column sum accumulated in fp32, its partial rows summed in float64 by the caller: per column
    |got - ref| <= (rows_per_lane + 8) x 2^-24 x sum_rows |term| (the lane's chain, then the folds across lanes / waves and
    the roundings inside a term). Returns the worst err / bound."""
    err = (got.double() - ref.double()).abs()
    bound = (rows_per_lane + 8) * 2.0 ** -24 * mag.double()
    bad = ~(torch.isfinite(got.double()) & (err <= bound))
    if bool(bad.any()):
        c = int(bad.nonzero()[0])
        raise AssertionError(f"{name}: column {c}: got {float(got[c])!r}, want {float(ref[c])!r}: off by {float(err[c]):.3e} > "
                             f"{rows_per_lane + 8} x 2^-24 x {float(mag[c]):.3e}; {int(bad.sum())} columns over")
    return float((err / bound.clamp_min(1e-300)).max())


LN_DY_KINDS = ("plain", "tiny", "spike", "zero")


def ln_dy(T, W, seed):
    """bf16 output gradients [T, W] on the CPU and the kind index per row: N(0,1); N(0,1) x 2^-14; N(0,1) with one element
    x 50 at column (r * 53) % W; an all-zero row (its dx row must be exactly zero). Kind (r + r // 6) % 4: every kind
    meets every one of the six backward input classes within 24 rows."""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(T, W, generator=g)
    r = torch.arange(T)
    kind = (r + r // 6) % 4
    dy[kind == 1] *= 2.0 ** -14
    sp = (kind == 2).nonzero().flatten()
    dy[sp, (sp * 53) % W] *= 50.0
    dy[kind == 3] = 0.0
    return dy.to(torch.bfloat16), kind


# ---- the AdamW element contract (tests/test_gpu_adamw_elements.py, tests/test_adamw_elements_host.py) ----------------------
# Every element of p, m and v that plb_launch_adamw / plb_launch_adamw_clipped store is held to one step in float64 from the
# same fp32 inputs, all scalars in double, within an allowance that counts the roundings of the kernel's operation list
# (csrc/optim.hip) and the one rounding of each host scalar, u = 2^-24:
#     tol_m = 4u (|m| + |gj|)      tol_v = 8u v'  (v' = 0: exactly 0)      tol_p = 4u |p| + 20u |upd| + (lr / bc1) / den x tol_m
# Nothing below calls a kernel or reads a kernel's output to form a bound; everything is numpy on the CPU.
ADAMW_U = 2.0 ** -24
ADAMW_B1, ADAMW_B2, ADAMW_EPS = 0.9, 0.999, 1e-8
ADAMW_TRIPLES = ((7e-5, 0.01, 1.0), (1e-3, 0.01, 0.125), (1e-3, 0.0, 1.0))     # (lr, wd, grad_scale)
ADAMW_DECAY_TRIPLE = (1e-2, 0.1, 1.0)    # decay before / after the update differ by lr x wd = 1e-3 of the update
ADAMW_STEPS = (1, 2, 10, 1000, 100000)
ADAMW_FLOOR = 1e-30                      # no non-zero intermediate of the reference is below it: subnormals are not the subject
ADAMW_BIG = 2e4                          # the sparse set of large parameters (what a norm over the range is made of)


def adamw_state(n, seed=2024, shared_exponent=True):
    """(p, g, m, v) float32 numpy [n]. p N(0, 0.05), every 53rd exactly 0, every 257th x 2e4; g N(0,1) exp(N(-6,4)), every
    97th 0; m N(0,1) exp(N(-7,3)), every 31st 0; v exp(N(-14,7)), every 41st 0, every 89th (+5) 1e-30 where g != 0 (sqrt(v)
    far below eps); every 211th (+7) element has g = m = v = 0: its update is exactly 0.
    m and v share the draw of their exponent (m = N(0,1) exp(3z - 7), v = exp(7z - 14)): the marginals are the ones above
    and |m| / sqrt(v) stays within a few tens, as in any state AdamW itself produced; where v is 0 or 1e-30, m is N(0,1) x
    1e-8, on the scale of eps. Drawn independently (shared_exponent=False), m / sqrt(v) reaches 10^7, the parameter range
    is made of updates, and a whole-range norm then does see a wrong decay (tests/test_adamw_elements_host.py)."""
    import numpy as np
    r = np.random.RandomState(seed)
    i = np.arange(n)
    p = r.standard_normal(n) * 0.05
    g = r.standard_normal(n) * np.exp(r.standard_normal(n) * 4.0 - 6.0)
    z = r.standard_normal(n)
    m = r.standard_normal(n) * np.exp(z * 3.0 - 7.0)
    v = np.exp((z if shared_exponent else r.standard_normal(n)) * 7.0 - 14.0)
    p[i % 257 == 3] *= ADAMW_BIG
    p[i % 53 == 0] = 0.0
    g[i % 97 == 0] = 0.0
    v[i % 41 == 0] = 0.0
    p, g, m, v = (a.astype(np.float32) for a in (p, g, m, v))
    v[(i % 89 == 5) & (g != 0) & (v != 0)] = np.float32(1e-30)
    edge = v <= np.float32(1e-30)
    m[edge] = (r.standard_normal(n) * 1e-8).astype(np.float32)[edge]
    m[i % 31 == 0] = 0.0
    still = i % 211 == 7
    g[still], m[still], v[still] = 0.0, 0.0, 0.0
    return p, g, m, v


def bf16_rne_bits(x):
    """The bf16 bit patterns (uint16) of float32 numpy values rounded to nearest, ties to even (finite values)."""
    import numpy as np
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


class AdamwRef:
    """adamw_fp64's results: the new p, m, v, the intermediates and the three allowances, float64 [n]."""
    __slots__ = ("p", "m", "v", "gj", "upd", "den", "decay", "tol_p", "tol_m", "tol_v", "p_in")


def adamw_fp64(p, g, m, v, lr, wd, gs, step, coef=None, b1=ADAMW_B1, b2=ADAMW_B2, eps=ADAMW_EPS):
    """One AdamW step in float64 from the fp32 inputs, every scalar in double; coef: the clipped form's (g gs) coef. Asserts
    that no non-zero intermediate is below ADAMW_FLOOR."""
    import numpy as np
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    o = AdamwRef()
    o.p_in = p
    o.gj = g * gs if coef is None else (g * gs) * float(coef)
    o.m = m + (1.0 - b1) * (o.gj - m)
    o.v = b2 * v + (1.0 - b2) * o.gj * o.gj
    o.den = np.sqrt(o.v) / np.sqrt(bc2) + eps
    o.upd = (lr / bc1) * o.m / o.den
    o.decay = 1.0 - lr * wd
    o.p = p * o.decay - o.upd
    for name, a in (("gj", o.gj), ("gj - m", o.gj - m), ("m'", o.m), ("gj^2", o.gj * o.gj), ("v'", o.v), ("upd", o.upd),
                    ("p decay", p * o.decay)):
        nz = np.abs(a[a != 0])
        assert nz.size == 0 or float(nz.min()) >= ADAMW_FLOOR, f"{name}: a non-zero intermediate of {float(nz.min()):.3e}"
    u = ADAMW_U
    o.tol_m = 4 * u * (np.abs(m) + np.abs(o.gj))
    o.tol_v = 8 * u * o.v
    o.tol_p = 4 * u * np.abs(p) + 20 * u * np.abs(o.upd) + (lr / bc1) / o.den * o.tol_m
    return o


def adamw_f32_restatement(p, g, m, v, lr, wd, gs, step, coef=None, fused=False, defect=None, b1=ADAMW_B1, b2=ADAMW_B2,
                          eps=ADAMW_EPS):
    """adamw_kernel's operation list (csrc/optim.hip) in numpy float32, the scalars formed in double and rounded once as the
    launcher forms them. fused: g gs - m as ONE operation (the contraction hipcc makes in adamw_kernel). defect: one of the
    planted faults of tests/test_adamw_elements_host.py ("omb2", "step+1", "no_sqrt_bc2", "eps_inside", "decay_after").
    Returns (p', m', v') float32."""
    import numpy as np
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    st = step + 1 if defect == "step+1" else step
    bc1, bc2 = 1.0 - b1 ** st, 1.0 - b2 ** st
    decay, omb1, b2f, epsf = f(1.0 - lr * wd), f(1.0 - b1), f(b2), f(eps)
    omb2 = f(1.0) - f(b2) if defect == "omb2" else f(1.0 - b2)
    stepf, bc2s, gsf = f(lr / bc1), f(np.sqrt(bc2)), f(gs)
    gj = g * gsf
    if coef is not None:
        gj = gj * f(coef)
    if fused and coef is None:
        d = (g.astype(np.float64) * np.float64(gsf) - m.astype(np.float64)).astype(f)
    else:
        d = gj - m
    m1 = m + omb1 * d
    v1 = b2f * v + omb2 * (gj * gj)
    if defect == "no_sqrt_bc2":
        den = np.sqrt(v1) + epsf
    elif defect == "eps_inside":
        den = (np.sqrt(v1) + epsf) / bc2s
    else:
        den = np.sqrt(v1) / bc2s + epsf
    if defect == "decay_after":
        p1 = (p - stepf * (m1 / den)) * decay
    else:
        p1 = p * decay - stepf * (m1 / den)
    return p1.astype(f), m1.astype(f), v1.astype(f)


def adamw_offender(got_p, got_m, got_v, ref, limit=1.0):
    """(ratios, offender): ratios = {"p", "m", "v": the worst |got - ref| / allowance}; offender = None, or (array name,
    index, got, want, allowance) of the FIRST element — m, then v, then p, lowest index — that is not finite, is over
    limit x its allowance, or is not exactly 0 where v' = 0."""
    import numpy as np
    ratios, offender = {}, None
    for name, got, want, tol in (("m", got_m, ref.m, ref.tol_m), ("v", got_v, ref.v, ref.tol_v), ("p", got_p, ref.p, ref.tol_p)):
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        err = np.abs(got - want)
        exact = tol == 0
        bad = ~np.isfinite(got) | np.where(exact, err != 0, err > limit * tol)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(exact, 0.0, err / np.where(exact, 1.0, tol))
        ratios[name] = float(r.max()) if r.size else 0.0
        if offender is None and bad.any():
            i = int(np.flatnonzero(bad)[0])
            offender = (name, i, float(got[i]), float(want[i]), float(tol[i]))
    return ratios, offender


def check_adamw(what, got_p, got_m, got_v, ref, limit=1.0):
    """Raises AssertionError naming the first offending element; returns the worst share of each allowance in use. Where
    g = m = v = 0 the update is exactly 0: m' = v' = 0 and p' = fl(p x fl(decay)), whichever contraction the compiler made."""
    import numpy as np
    ratios, off = adamw_offender(got_p, got_m, got_v, ref, limit)
    if off is not None:
        name, i, got, want, tol = off
        raise AssertionError(f"{what}: {name}[{i}] (float4 {i // 4} component {i % 4}, workgroup {i // 1024}): got {got!r}, "
                             f"want {want!r}: off by {abs(got - want):.3e} > {limit:g} x {tol:.3e}")
    still = (ref.gj == 0) & (ref.m == 0) & (ref.v == 0)
    want = (ref.p_in.astype(np.float32) * np.float32(ref.decay)).astype(np.float32)
    bad = still & (np.asarray(got_p, dtype=np.float32) != want)
    assert not bad.any(), f"{what}: p[{int(np.flatnonzero(bad)[0])}] has a zero update and is not p x decay"
    return ratios


def check_bf16_copy(what, pb_bits, p_out):
    """The bf16 copy (uint16 bit patterns) must be the round-to-nearest-even of the fp32 p the SAME launch stored, at every
    element, bit for bit."""
    import numpy as np
    want = bf16_rne_bits(p_out)
    got = np.asarray(pb_bits).view(np.uint16) if np.asarray(pb_bits).dtype != np.uint16 else np.asarray(pb_bits)
    bad = got != want
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: bf16 copy [{i}]: got 0x{int(got[i]):04x}, want 0x{int(want[i]):04x} for p = "
                             f"{float(np.asarray(p_out)[i])!r}; {int(bad.sum())} elements differ")


def bf16_tie_values():
    """float32 values exactly half way between two bf16 numbers, both signs: the even neighbour below (round down), the even
    neighbour above (round up), at several exponents; and the values one fp32 step either side of each tie."""
    import numpy as np
    out = []
    for hi in (0x3F80, 0x3F81, 0x4000, 0x4049, 0x3DCC, 0x3DCD, 0x2000, 0x7F00, 0x3FFF):
        for sign in (0, 0x8000):
            for low in (0x8000, 0x7FFF, 0x8001):
                out.append(((hi | sign) << 16) | low)
    return np.array(out, dtype=np.uint32).view(np.float32)
