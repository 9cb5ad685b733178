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


def gemm_nt(A, B, N, bias=None, res=None, aux=None, act=0, out_f32=False, Mstore=None, ldout=None):
    """A [M,K] bf16, B [>=ceil128(N),K] bf16 -> C (bf16 or fp32) [M, ldout]."""
    L = _lib.lib()
    M, K = A.shape
    ldout = ldout or N
    dev = A.device
    Cb = torch.zeros((M, ldout), dtype=torch.bfloat16, device=dev)
    C2 = torch.zeros((M, ldout), dtype=torch.bfloat16, device=dev)
    Cf = torch.zeros((M, ldout), dtype=torch.float32, device=dev)
    p = _lib.PlbGemmNT()
    p.A, p.lda, p.B, p.ldb = A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0)
    p.M, p.N, p.K, p.Mstore = M, N, K, (M if Mstore is None else Mstore)
    p.bias = bias.data_ptr() if bias is not None else None
    if res is not None:
        p.res, p.ldr = res.data_ptr(), res.stride(0)
    if aux is not None:
        p.aux, p.ldaux = aux.data_ptr(), aux.stride(0)
    p.C, p.ldc, p.C2, p.ldc2, p.Cf, p.ldcf = Cb.data_ptr(), ldout, C2.data_ptr(), ldout, Cf.data_ptr(), ldout
    rc = L.plb_launch_gemm_nt(C.byref(p), act, int(out_f32), stream())
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


# ---- raw launchers of the row and fp8 kernels (csrc/plbert_kernels.h) --------------------------------------------------
# ctypes passes a Python int as a C int unless told otherwise: a size_t or float parameter would then receive garbage in
# its upper bits / the bit pattern of an int. bind() declares the launchers the kernel-level tests call with scalar
# arguments that plbert_amd/_lib.py leaves undeclared; struct-taking launchers are called with C.byref(struct).
_vp, _i, _sz, _f = C.c_void_p, C.c_int, C.c_size_t, C.c_float
_SIGNATURES = {
    "plb_launch_amax": [_vp, _i, _sz, _i, _i, _vp, _vp],
    "plb_launch_fp8_scales": [_vp, _vp, _vp, _i, _f, _i, _vp],
    "plb_launch_fp8_scales2": [_vp, _vp, _vp, _i, _f, _i, _i, _f, _vp, _i, _vp],
    "plb_launch_quantize": [_vp, _i, _sz, _i, _i, _vp, _vp, _i, _i, _vp],
    "plb_launch_quantize_multi": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "plb_launch_copy_cols": [_vp, _i, _i, _i, _i, _vp, _vp],
    "plb_launch_pooler": [_vp, _i, _i, _i, _vp, _vp, _vp, _vp],
    "plb_launch_gather_rows": [_vp, _i, _vp, _i, _i, _i, _vp, _i, _vp],
    "plb_launch_scatter_rows": [_vp, _i, _vp, _i, _i, _vp, _i, _vp],
    "plb_launch_ce_prepare": [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp],
    "plb_launch_ce_fwd_bwd": [_vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _vp],
    "plb_launch_sum_rows": [_vp, _i, _vp, _vp],
    "plb_launch_cast_bf16": [_vp, _vp, _sz, _vp],
    "plb_launch_transpose_cast": [_vp, _i, _i, _vp, _i, _vp],
    "plb_launch_transpose_cast_multi": [_i, _vp, _vp, _vp, _vp, _vp, _vp],
    "plb_launch_bf16_to_f32": [_vp, _i, _vp, _i, _i, _i, _vp],
}


def bind(L=None):
    """Declare restype / argtypes of the scalar-argument launchers; returns the library."""
    L = L or _lib.lib()
    for name, args in _SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = C.c_int
        fn.argtypes = args
    return L


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
