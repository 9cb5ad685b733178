"""-m gpu: the attention kernels with key masks (PlbAttn.key_words), at kernel level through plb_launch_attn_*.

The masked instantiations of the forward, dQ and dK/dV kernels (csrc/attn_kernels.h, ATTN_KM 1) take the valid keys from
one bit per key (csrc/key_mask.hip packs them). Every (row, head) of ctx, dq, dk and dv is held to keymask_ref.attention_fp64
within gpu_util.ROW_FACTOR x the worst row of keymask_ref.attention_rounded on the same inputs — the contract of
test_gpu_attention_rows.py, with a mask in the place of a length; lse per element (2e-3); delta per row (check_delta); dk / dv
rows of masked keys and every gradient row past the extent exactly zero; nothing NaN or Inf; the number of (row, head)
pairs under the absolute check as the mask predicts (a sample with ONE valid key has P = 1, so dq of its rows and dk of that
key are zero in the reference).

Cases (NH 2):
    holes     8 x 256   one hole per sample, at key 0, 31, 32, 63, 64, 127, 128, 255
    leftpad   8 x 192   left pads of 1, 31, 32, 33, 64, 65, 128, 191 keys (191 leaves one valid key)
    empty     4 x 256   keys without a bit: an aligned 32-key group [96,128); a 64-key tile [64,128); the 128-key block
                        [0,128) (S = 256 has two such blocks: the first one is masked, so a whole dK/dV workgroup has no key
                        and the forward's first two tiles are empty); all three at once ([0,128) + [128,192) + [192,224))
    random    3 x 130   Bernoulli(0.5), extents 130 / 129 / 40
    single    2 x 192   one valid key, at 0 and at 77

Maxima of the row error (model: attention_rounded against attention_fp64, evaluated where the test runs; kernel: the masked
kernels, measured on an MI355X). The -s run prints `keymask <case>: <output> model <max> kernel <max>`:

    case      ctx  model | kernel     dq  model | kernel      dk  model | kernel      dv  model | kernel
    holes     3.228e-03  3.887e-03    3.878e-03  4.939e-03    3.981e-03  3.939e-03    4.028e-03  4.028e-03
    leftpad   3.308e-03  4.188e-03    4.910e-03  5.219e-03    3.747e-03  3.734e-03    3.620e-03  3.620e-03
    empty     3.219e-03  3.362e-03    4.268e-03  6.168e-03    4.538e-03  3.979e-03    3.387e-03  3.387e-03
    random    3.021e-03  3.329e-03    5.167e-03  5.167e-03    3.591e-03  3.618e-03    3.479e-03  3.479e-03
    single    0          0            0          4.508e-07    0          1.788e-06    1.790e-03  1.790e-03
  single: one valid key per sample, so ctx is the key's V row exactly and the references of dq and dk are zero: their kernel
  columns are the largest |value| (rows_check's absolute rule, ROW_ABS = 1e-5).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import keymask_ref as R
from plbert_amd import _lib
from gpu_util import ATTN_SCALE, ROW_ABS, attention_delta_terms, attn_args, check_delta, check_rows, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
NH, H = 2, 128


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def _ones(B, S):
    return torch.ones(B, S, dtype=torch.int32)


def mask_holes():
    m = _ones(8, 256)
    for b, j in enumerate([0, 31, 32, 63, 64, 127, 128, 255]):
        m[b, j] = 0
    return m


def mask_leftpad():
    m = _ones(8, 192)
    for b, n in enumerate([1, 31, 32, 33, 64, 65, 128, 191]):
        m[b, :n] = 0
    return m


def mask_empty():
    m = _ones(4, 256)
    m[0, 96:128] = 0
    m[1, 64:128] = 0
    m[2, 0:128] = 0
    m[3, 0:224] = 0
    return m


def mask_random():
    m = (torch.rand(3, 130, generator=torch.Generator().manual_seed(7)) < 0.5).to(torch.int32)
    for b, n in enumerate([130, 129, 40]):
        m[b, n - 1] = 1
        m[b, n:] = 0
    return m


def mask_single():
    m = torch.zeros(2, 192, dtype=torch.int32)
    m[0, 0] = 1
    m[1, 77] = 1
    return m


CASES = {"holes": mask_holes, "leftpad": mask_leftpad, "empty": mask_empty, "random": mask_random, "single": mask_single}
_REFS = {}   # case -> inputs, float64 reference and rounding model: evaluated once, shared, never modified


def pack_words(mask, lengths, B, S, ldkw=None, tail=0):
    """plb_launch_key_mask_words on a sentinel-filled buffer of B * ldkw + tail words."""
    ldkw = R.row_stride(S) if ldkw is None else ldkw
    buf = torch.full((B * ldkw + tail,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rc = _lib.lib().plb_launch_key_mask_words(mask.data_ptr(), None if lengths is None else lengths.data_ptr(), B, S,
                                              buf.data_ptr(), ldkw, stream())
    assert rc == 0, rc
    return buf, ldkw


def reference(name):
    if name not in _REFS:
        mask = CASES[name]()
        B, S = mask.shape
        ext = R.extents(mask).to(torch.int32)
        g = dict(B=B, S=S, mask=mask.to(DEV), lengths=ext.to(DEV), ext=ext.tolist())
        g["qkv"] = randn(B * S, 3 * H, seed=300 + list(CASES).index(name)).to(torch.bfloat16).to(DEV)
        g["inside"] = (torch.arange(S, device=DEV)[None, :] < g["lengths"][:, None]).reshape(B * S)
        g["keys"] = R.valid_keys(g["mask"], g["lengths"], S).reshape(B * S)
        # dO is zero at and past the extent, as in the model (no loss there); a hole has its own dO: it is a query
        g["dctx"] = (randn(B * S, H, seed=400 + list(CASES).index(name)).to(DEV) * g["inside"][:, None]).to(torch.bfloat16)
        for key, fn in (("ref", R.attention_fp64), ("mod", R.attention_rounded)):
            out = {}
            out["ctx"], out["lse"], grad = fn(g["qkv"], g["mask"], g["lengths"], B, S, NH)
            out["dq"], out["dk"], out["dv"], _ = grad(g["dctx"])
            g[key] = out
        _REFS[name] = g
    return _REFS[name]


def run(qkv, lengths, B, S, dctx, words=None, ldkw=0, row_start=None, rows=None, colpart=False):
    """Forward + backward through plb_launch_attn_fwd / _bwd. Returns ctx, lse, delta, dqkv (+ colpart)."""
    L = _lib.lib()
    p, ctx, lse = attn_args(qkv, lengths, B, S, NH)
    if rows is not None:
        ctx = torch.zeros((rows, H), dtype=torch.bfloat16, device=DEV)
        p.ctx = ctx.data_ptr()
        p.row_start = row_start.data_ptr()
    if words is not None:
        p.key_words, p.ldkw = words.data_ptr(), ldkw
    assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 0
    delta = torch.zeros((B, NH, S), dtype=torch.float32, device=DEV)
    dqkv = torch.full((ctx.shape[0], 3 * H), 7.0, dtype=torch.bfloat16, device=DEV)
    p.dctx, p.lddctx, p.delta, p.dqkv, p.lddqkv = dctx.data_ptr(), H, delta.data_ptr(), dqkv.data_ptr(), 3 * H
    cp = None
    if colpart:
        cp = torch.full((B * ((S + 127) // 128) * 4, 3 * H), 3.0, dtype=torch.float32, device=DEV)
        p.colpart = cp.data_ptr()
    assert L.plb_launch_attn_bwd(C.byref(p), stream()) == 0
    torch.cuda.synchronize()
    return ctx, lse, delta, dqkv, cp


def rows_check(what, got, ref, model, valid, n_abs):
    """gpu_util.check_rows; an output whose reference is zero on EVERY valid row (dq and dk of the `single` case: one valid key
    per sample, P = 1, dS = 0) has no largest row to call a row tiny against, so all its valid rows go under check_rows'
    absolute rule directly: |got| < ROW_ABS there, exact zeros elsewhere, and their number as predicted."""
    den = ref.double().reshape(-1, NH, 64).norm(dim=-1)[valid]
    if float(den.max()) > 0.0:
        return check_rows(what, got, ref, model, NH, valid=valid, n_abs=n_abs)
    g = got.double()[:ref.shape[0]]
    assert int(valid.sum()) * NH == n_abs, (what, int(valid.sum()) * NH, n_abs)
    assert bool((g[~valid] == 0).all()), f"{what}: a padded row is not exactly zero"
    assert float(g[valid].abs().max()) < ROW_ABS, (what, float(g[valid].abs().max()))
    return {"model": 0.0, "got": float(g[valid].abs().max()), "bound": ROW_ABS, "n_abs": n_abs}


@pytest.mark.parametrize("name", list(CASES))
def test_attention_keymask_rows(name):
    """One case through the masked kernels (module docstring: the contract and the figures)."""
    c = reference(name)
    B, S = c["B"], c["S"]
    ref, mod = c["ref"], c["mod"]
    words, ldkw = pack_words(c["mask"], c["lengths"], B, S)
    ctx, lse, delta, dqkv, _ = run(c["qkv"], c["lengths"], B, S, c["dctx"], words, ldkw)
    for t in (ctx, lse, delta, dqkv):
        assert bool(torch.isfinite(t.float()).all())
    # a sample with one valid key: P = 1 on it, dP - delta = 0, so dq of its rows and dk of that key are 0 in the reference
    one = [b for b in range(B) if int(c["keys"].reshape(B, S)[b].sum()) == 1]
    fig = {}
    fig["ctx"] = check_rows("ctx", ctx, ref["ctx"], mod["ctx"], NH)
    fig["dq"] = rows_check("dq", dqkv[:, :H], ref["dq"], mod["dq"], c["inside"], NH * sum(c["ext"][b] for b in one))
    fig["dk"] = rows_check("dk", dqkv[:, H:2 * H], ref["dk"], mod["dk"], c["keys"], NH * len(one))
    fig["dv"] = check_rows("dv", dqkv[:, 2 * H:], ref["dv"], mod["dv"], NH, valid=c["keys"])
    print(f"keymask {name:8s}:" + "".join(f"  {k} model {v['model']:.3e} kernel {v['got']:.3e}" for k, v in fig.items()))
    assert float((-lse.double() * ATTN_SCALE - ref["lse"]).abs().max()) <= 2e-3
    check_delta(delta, *attention_delta_terms(c["dctx"], ctx, B, S, NH))


@pytest.fixture
def split_form():
    """The namesake runs in the two-kernel form, as a call with words always does; afterwards the per-shape policy is back."""
    L = _lib.lib()
    L.plb_set_attn_bwd_fused(0)
    yield
    L.plb_set_attn_bwd_fused(-1)


def _same(a, b, what):
    assert all(torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32),
                           y.view(torch.int16) if y.dtype == torch.bfloat16 else y.view(torch.int32))
               for x, y in zip(a, b)), what


@pytest.mark.parametrize("B,S,lens", [(3, 130, [130, 129, 40]), (2, 256, [256, 193]), (2, 192, None)])
def test_all_ones_and_prefix_words_are_bit_equal_to_the_lengths_only_call(split_form, B, S, lens):
    """The masked kernels do the same arithmetic per row: an all-ones mask with these lengths, and the prefix mask itself, give
    ctx, lse, delta, dq, dk, dv and colpart of the call without words bit for bit."""
    qkv = randn(B * S, 3 * H, seed=501).to(torch.bfloat16).to(DEV)
    lengths = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    inside = torch.ones(B * S, dtype=torch.bool, device=DEV) if lens is None else \
        (torch.arange(S, device=DEV)[None, :] < lengths[:, None]).reshape(B * S)
    dctx = (randn(B * S, H, seed=502).to(DEV) * inside[:, None]).to(torch.bfloat16)
    plain = run(qkv, lengths, B, S, dctx, colpart=True)
    ones = _ones(B, S).to(DEV)
    prefix = inside.reshape(B, S).to(torch.int32)
    for what, m in (("all-ones mask", ones), ("prefix mask", prefix)):
        words, ldkw = pack_words(m, lengths, B, S)
        _same(run(qkv, lengths, B, S, dctx, words, ldkw, colpart=True), plain, what)


def test_forced_single_kernel_form_still_takes_the_two_kernel_form_with_words():
    """plb_set_attn_bwd_fused(1) with words: the call passes through the dQ and dK/dV kernels (delta is written: the
    single-kernel form keeps it in LDS) and gives the bits of the two-kernel policy."""
    c = reference("holes")
    B, S = c["B"], c["S"]
    words, ldkw = pack_words(c["mask"], c["lengths"], B, S)
    L = _lib.lib()
    try:
        L.plb_set_attn_bwd_fused(0)
        want = run(c["qkv"], c["lengths"], B, S, c["dctx"], words, ldkw, colpart=True)
        L.plb_set_attn_bwd_fused(1)
        got = run(c["qkv"], c["lengths"], B, S, c["dctx"], words, ldkw, colpart=True)
    finally:
        L.plb_set_attn_bwd_fused(-1)
    assert bool((got[2] != 0).any())
    _same(got, want, "forced single-kernel form")


def test_words_with_compact_queries_or_a_short_row_are_refused():
    c = reference("random")
    B, S = c["B"], c["S"]
    words, ldkw = pack_words(c["mask"], c["lengths"], B, S)
    p, _, _ = attn_args(c["qkv"], c["lengths"], B, S, NH)
    p.key_words, p.ldkw = words.data_ptr(), ldkw - 1
    assert _lib.lib().plb_launch_attn_fwd(C.byref(p), stream()) == 1
    p.ldkw = ldkw
    qoff = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    p.qoff, p.q, p.ldq, p.nq_total = qoff.data_ptr(), c["qkv"].data_ptr(), 3 * H, 0
    assert _lib.lib().plb_launch_attn_fwd(C.byref(p), stream()) == 1


def test_packed_rows_with_holes_equal_the_padded_call():
    """row_start with holes: every valid row of ctx and dqkv, and lse / delta (indexed by (b, S) in both layouts), are the
    padded call's bit for bit."""
    c = reference("random")
    B, S, ext = c["B"], c["S"], c["ext"]
    words, ldkw = pack_words(c["mask"], c["lengths"], B, S)
    pad = run(c["qkv"], c["lengths"], B, S, c["dctx"], words, ldkw)
    starts, n = [], 0
    for e in ext:
        starts.append(n)
        n += (e + 127) // 128 * 128
    row_start = torch.tensor(starts, dtype=torch.int32, device=DEV)
    src = torch.cat([torch.arange(e) + b * S for b, e in enumerate(ext)]).to(DEV)
    dst = torch.cat([torch.arange(e) + starts[b] for b, e in enumerate(ext)]).to(DEV)
    qkv = torch.zeros((n, 3 * H), dtype=torch.bfloat16, device=DEV)
    dctx = torch.zeros((n, H), dtype=torch.bfloat16, device=DEV)
    qkv[dst], dctx[dst] = c["qkv"][src], c["dctx"][src]
    got = run(qkv, c["lengths"], B, S, dctx, words, ldkw, row_start=row_start, rows=n)
    inside = c["inside"].reshape(B, S)[:, None, :].expand(B, NH, S)
    _same((got[0][dst], got[3][dst], got[1][inside], got[2][inside]), (pad[0][src], pad[3][src], pad[1][inside], pad[2][inside]),
          "packed rows")


@pytest.mark.parametrize("S", [1, 31, 32, 33, 40, 64, 65, 130, 192, 2048])
def test_key_mask_words_equal_the_numpy_restatement(S):
    """The packing kernel against keymask_ref.key_words_np bit for bit: lengths given and NULL, a row stride wider than
    needed (the words behind 2 * ceil(S / 64) of a row are not written), a sentinel behind the buffer."""
    B = 5
    g = torch.Generator().manual_seed(S)
    mask = (torch.rand(B, S, generator=g) < 0.6).to(torch.int32) * 3
    lens = torch.tensor([S, max(S - 1, 1), (S + 1) // 2, 1, 0], dtype=torch.int32)   # 0: clamped to 1, as everywhere
    for lengths in (lens, None):
        for extra in (0, 3):
            ldkw = R.row_stride(S) + extra
            buf, _ = pack_words(mask.to(DEV), None if lengths is None else lengths.to(DEV), B, S, ldkw=ldkw, tail=8)
            torch.cuda.synchronize()
            got = buf.cpu().numpy().view(np.uint32)
            want = R.key_words_np(mask.numpy(), None if lengths is None else lengths.numpy(), S)
            rows = got[:B * ldkw].reshape(B, ldkw)
            assert np.array_equal(rows[:, :R.row_stride(S)], want)
            assert (rows[:, R.row_stride(S):] == 0x5A5A5A5A).all() and (got[B * ldkw:] == 0x5A5A5A5A).all()
    assert _lib.lib().plb_launch_key_mask_words(mask.to(DEV).data_ptr(), None, B, S, buf.data_ptr(), R.row_stride(S) - 1, stream()) == 1


@pytest.mark.parametrize("name", ["holes", "random", "empty"])
def test_attn_probs_with_words(name):
    """plb_launch_attn_probs_masked: hole columns, columns and rows past the extent are exact zeros; the rows below the extent
    (holes among them) sum to 1 within the bound tests/test_gpu_layer_outputs.py holds that sum to (3e-3) and follow the
    float64 softmax; every element is written (the buffer starts as NaN)."""
    c = reference(name)
    B, S = c["B"], c["S"]
    L = _lib.lib()
    words, ldkw = pack_words(c["mask"], c["lengths"], B, S)
    p, ctx, lse = attn_args(c["qkv"], c["lengths"], B, S, NH)
    p.key_words, p.ldkw = words.data_ptr(), ldkw
    assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 0
    out = torch.full((B, NH, S, S), float("nan"), dtype=torch.float32, device=DEV)
    assert L.plb_launch_attn_probs_masked(c["qkv"].data_ptr(), 3 * H, lse.data_ptr(), c["lengths"].data_ptr(), None,
                                          words.data_ptr(), ldkw, B, S, NH, 0.125, out.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    keys, inside = c["keys"].reshape(B, S), c["inside"].reshape(B, S)
    assert bool(torch.isfinite(out).all())
    assert bool((out[~keys[:, None, None, :].expand_as(out)] == 0).all())
    assert bool((out[~inside[:, None, :, None].expand_as(out)] == 0).all())
    rows = inside[:, None, :].expand(B, NH, S)
    assert float((out.double().sum(-1)[rows] - 1).abs().max()) <= 3e-3
    want = R.probs_fp64(c["qkv"], c["mask"], c["lengths"], B, S, NH)
    assert float((out.double() - want)[rows].abs().max()) <= 3e-3
    # without words the launcher is the one it always was
    out2 = torch.full_like(out, float("nan"))
    ones, _ = pack_words(_ones(B, S).to(DEV), c["lengths"], B, S)
    p2, _, lse2 = attn_args(c["qkv"], c["lengths"], B, S, NH)
    assert L.plb_launch_attn_fwd(C.byref(p2), stream()) == 0
    assert L.plb_launch_attn_probs(c["qkv"].data_ptr(), 3 * H, lse2.data_ptr(), c["lengths"].data_ptr(), None, B, S, NH, 0.125,
                                   out.data_ptr(), stream()) == 0
    assert L.plb_launch_attn_probs_masked(c["qkv"].data_ptr(), 3 * H, lse2.data_ptr(), c["lengths"].data_ptr(), None,
                                          ones.data_ptr(), ldkw, B, S, NH, 0.125, out2.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
