"""The attention launchers against their plan (csrc/attn_plan.h), on the GPU, at the smallest shapes that reach every branch:
buffers sized by the plan's counts plus sentinel guards are written exactly where the plan says — every planned partial row,
no guard, no row of a packed slot at or past position S (the plan's unwritten_rows) — and a refused launch leaves no
profiler record open."""
import ctypes as C
import functools

import pytest
import torch

from plbert_amd import _lib
from gpu_util import attn_args, rel_l2, stream, torch_attention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT, SENT16 = 1.2345e30, -123.0   # fp32 partial rows and statistics; bf16 rows (exact in bf16)
TWO, ONE = 0, 1


@functools.lru_cache(maxsize=None)
def inputs(B, S, NH, lens):
    """qkv and dctx of the padded call (dctx zero on padded queries, as in the model) and the reference gradient."""
    H = NH * 64
    g = torch.Generator(device="cpu").manual_seed(7 * B + S)
    qkv = torch.randn(B * S, 3 * H, generator=g).to(torch.bfloat16).to(DEV)
    dctx = torch.randn(B * S, H, generator=g).to(torch.bfloat16).to(DEV)
    lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
    valid = (torch.arange(S, device=DEV)[None, :] < lengths[:, None]).reshape(B * S)
    dctx = dctx * valid[:, None].to(dctx.dtype)
    ref = torch_attention(qkv, lengths, B, S, NH)[2](dctx)
    return qkv, dctx, lengths, valid, ref


def run(B, S, NH, lens, packed, form):
    """Forward and backward on buffers sized by the plan; returns what the checks below read."""
    L = _lib.lib()
    H = NH * 64
    qkv, dctx, lengths, valid, ref = inputs(B, S, NH, lens)
    slot = [(n + 127) // 128 * 128 for n in lens]
    start = [sum(slot[:b]) for b in range(B + 1)]
    if packed:   # sample b's tokens at rows start[b]..; the rest of a slot holds finite rows of no token
        rows = torch.cat([torch.arange(min(slot[b], S)) + b * S for b in range(B)]).to(DEV)
        at = torch.cat([torch.arange(min(slot[b], S)) + start[b] for b in range(B)]).to(DEV)
        T = start[B]
        q_in = torch.zeros(T, 3 * H, dtype=torch.bfloat16, device=DEV)
        d_in = torch.zeros(T, H, dtype=torch.bfloat16, device=DEV)
        q_in[at], d_in[at] = qkv[rows], dctx[rows]
    else:
        T, q_in, d_in = B * S, qkv, dctx
    p, _, _ = attn_args(q_in, lengths, B, S, NH)
    row_start = torch.tensor(start, dtype=torch.int32, device=DEV)
    if packed:
        p.row_start = row_start.data_ptr()
    L.plb_set_attn_bwd_fused(form)
    try:
        plan = _lib.attn_plan(B, S, NH, (_lib.ATTN_PACKED if packed else 0) | _lib.ATTN_OUT_ROWS)
        assert plan["rc"] == 0
        ctx = torch.full((T, H), SENT16, dtype=torch.bfloat16, device=DEV)
        dqkv = torch.full((T, 3 * H), SENT16, dtype=torch.bfloat16, device=DEV)
        lse = torch.full((plan["stat_floats"] + 64,), SENT, device=DEV)
        delta = torch.full((plan["stat_floats"] + 64,), SENT, device=DEV)
        colp = torch.full((plan["colpart_rows"] + 8, 3 * H), SENT, device=DEV)
        p.ctx, p.lse = ctx.data_ptr(), lse.data_ptr()
        p.dctx, p.lddctx, p.delta, p.dqkv, p.lddqkv = d_in.data_ptr(), H, delta.data_ptr(), dqkv.data_ptr(), 3 * H
        p.colpart, p.colpart_accumulate = colp.data_ptr(), 0
        _lib.profile_enable(True)
        try:
            assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 0
            assert L.plb_launch_attn_bwd(C.byref(p), stream()) == 0
            torch.cuda.synchronize()
            launches = {k: v["launches"] for k, v in _lib.profile_read().items() if v["launches"]}
        finally:
            _lib.profile_enable(False)
    finally:
        L.plb_set_attn_bwd_fused(-1)
    # position of every row inside its sample's slot (padded: inside its sample)
    pos = torch.cat([torch.arange(slot[b] if packed else S) for b in range(B)]).to(DEV)
    tok = torch.cat([torch.arange(slot[b] if packed else S) < lens[b] for b in range(B)]).to(DEV)
    return dict(plan=plan, ctx=ctx, dqkv=dqkv, lse=lse, delta=delta, colp=colp, launches=launches, pos=pos, tok=tok, ref=ref[valid])


CASES = [
    # a tile that crosses S, a one-tile sample, a two-tile sample
    (3, 200, 2, (200, 77, 129), False, -1, TWO), (3, 200, 2, (200, 77, 129), True, -1, TWO),
    # the single kernel's range, both forms forced
    (2, 448, 2, (448, 300), False, 1, ONE), (2, 448, 2, (448, 300), False, 0, TWO),
    # a 1-row second tile
    (2, 129, 1, (129, 5), True, -1, TWO),
]


@pytest.mark.parametrize("B,S,NH,lens,packed,policy,form", CASES)
def test_the_launches_write_what_the_plan_counts(B, S, NH, lens, packed, policy, form):
    r = run(B, S, NH, lens, packed, policy)
    plan = r["plan"]
    QT = (S + 127) // 128
    assert (plan["bwd_form"], plan["colpart_rows"], plan["stat_floats"]) == (form, B * QT * 4, B * NH * S)
    assert r["launches"] == ({"attn_fwd": 1, "attn_bwd": 1} if form == ONE else {"attn_fwd": 1, "attn_bwd_dq": 1, "attn_bwd_dkv": 1})
    # partial rows: every planned row written, no guard row touched
    n = plan["colpart_rows"]
    assert not (r["colp"][:n] == SENT).any() and (r["colp"][n:] == SENT).all()
    # statistics: nothing past the plan's count; the forward of a padded call writes every one, the two kernels every delta
    n = plan["stat_floats"]
    assert (r["lse"][n:] == SENT).all() and (r["delta"][n:] == SENT).all()
    if not packed:
        assert not (r["lse"][:n] == SENT).any()
        assert (r["delta"][:n] == SENT).all() if form == ONE else not (r["delta"][:n] == SENT).any()
    # rows: positions at or past S of a packed slot are written by no launch, exactly where the plan says so
    unwritten = r["pos"] >= S
    assert plan["unwritten_rows"] == int(bool(unwritten.any())) == int(packed and S % 128 != 0)
    for name in ("ctx", "dqkv"):
        kept = (r[name] == SENT16).all(dim=1)
        assert torch.equal(kept, unwritten), name
        assert not (r[name][~unwritten] == SENT16).any(), name
    # and what they wrote is the gradient (the bias partial rows sum to the columns of the rows stored)
    got = r["dqkv"][r["tok"]].float()
    assert rel_l2(got, r["ref"]) < 1.5e-2
    stored = r["dqkv"][~unwritten].double().sum(0)
    assert torch.allclose(r["colp"][:plan["colpart_rows"]].double().sum(0), stored, rtol=1e-5, atol=1e-3 * float(r["ref"].abs().max()) * 10)


def single_kernel_descriptor():
    B, S, NH, lens = 2, 448, 2, (448, 300)
    H = NH * 64
    qkv, dctx, lengths, _, _ = inputs(B, S, NH, lens)
    p, ctx, lse = attn_args(qkv, lengths, B, S, NH)
    assert _lib.lib().plb_launch_attn_fwd(C.byref(p), stream()) == 0
    dqkv = torch.zeros(B * S, 3 * H, dtype=torch.bfloat16, device=DEV)
    p.dctx, p.lddctx, p.dqkv, p.lddqkv = dctx.data_ptr(), H, dqkv.data_ptr(), 3 * H
    return p, (ctx, lse, dqkv)


def test_a_refused_launch_opens_no_profiler_scope():
    """Rows AND image is refused by the single kernel's launcher. With profiling on, the launch that follows is recorded and
    read back: one attn_bwd, and plb_profile_read has no record without its end event."""
    L = _lib.lib()
    p, keep = single_kernel_descriptor()
    img = torch.zeros(2 * 448, 3 * 128, dtype=torch.uint8, device=DEV)
    scale = torch.tensor([512.0], device=DEV)
    _lib.profile_enable(True)
    try:
        p.dqkv8, p.lddqkv8, p.dqkv_scale = img.data_ptr(), 3 * 128, scale.data_ptr()
        assert L.plb_launch_attn_bwd_fused(C.byref(p), stream()) == 1
        p.dqkv8, p.lddqkv8, p.dqkv_scale = None, 0, None
        assert L.plb_launch_attn_bwd_fused(C.byref(p), stream()) == 0
        torch.cuda.synchronize()
        n = L.plb_profile_num_classes()
        ms, fl, by, cnt = (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)(), (C.c_int64 * n)()
        assert L.plb_profile_read(ms, cnt, fl, by) == 0
        names = [L.plb_profile_class_name(i).decode() for i in range(n)]
        assert {names[i]: cnt[i] for i in range(n) if cnt[i]} == {"attn_bwd": 1}
    finally:
        _lib.profile_enable(False)


def test_the_single_kernel_refuses_a_key_mask():
    L = _lib.lib()
    p, keep = single_kernel_descriptor()
    words = torch.full((2, 14), -1, dtype=torch.int32, device=DEV)   # (every key takes part)
    p.key_words, p.ldkw = words.data_ptr(), 14
    assert L.plb_attn_args_check(C.byref(p), 1) == 0       # the two kernels take it
    assert L.plb_launch_attn_bwd_fused(C.byref(p), stream()) == 1
