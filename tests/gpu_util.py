"""Helpers shared by the -m gpu tests: raw launches through the C ABI with torch tensors as buffers."""
import ctypes as C

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
