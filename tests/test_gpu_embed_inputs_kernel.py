"""The embedding launches with per-token sources (csrc/embed_inputs.hip) through ctypes (-m gpu): plb_launch_embed_inputs_fwd /
_bwd / _scatter against float64, against the plain launches of embed.hip when the defaults are passed explicitly, and the table
sums against the float64 sum of the dx rows the kernel itself wrote, element by element, within the bound of a fixed-order
fp32 sum: n * 2^-24 * sum|terms| (n = the element's term count; one term or none: exact)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import stream
from plbert_amd import _lib
from plbert_amd.engine import packing_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, P, NTY = 188, 512, 3
K_SHAPE = (5, 300, [300, 129, 128, 65, 1])     # 1500 padded positions: 3 chunks of 512, the last one short; its plan packs
CHUNKS = (3, 512, None)                        # 3 full chunks, no padding


def _tables(E, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(word=torch.randn(V, E, generator=g), pos=torch.randn(P, E, generator=g) * 0.5,
                type=torch.randn(NTY, E, generator=g) * 0.3, gamma=1 + 0.3 * torch.randn(E, generator=g),
                beta=0.2 * torch.randn(E, generator=g))


def _batch(E, shape, pattern, seed):
    """ids with a few hot ids and the padding id, token types, positions, inputs_embeds, the upstream gradient of the
    LayerNorm output (bf16, nonzero everywhere)."""
    B, S, lens = shape
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (B, S), generator=g)
    hot = torch.rand(B, S, generator=g)
    ids[hot < 0.3] = 3
    ids[(hot >= 0.3) & (hot < 0.4)] = 0
    tt = torch.randint(0, NTY, (B, S), generator=g)
    pid = torch.randint(0, P, (B, S), generator=g)
    if pattern == "one":        # every token on one type row and one position row; the other rows get exact zeros
        tt[:], pid[:] = 1, 77
    elif pattern == "unused":   # type row 1 and the position rows from 100 on belong to nobody
        tt[tt == 1] = 2
        pid %= 100
    xe = torch.randn(B, S, E, generator=g)
    return ids, tt, pid, xe, g


class Run:
    """One forward + backward + scatter through the launchers: sources=None runs the plain launchers of embed.hip."""

    def __init__(self, E, shape, packed, tb, ids, tt, pid, xe, dy, nblocks=64, want_die=True):
        L = _lib.lib()
        B, S, lens = shape
        self.plan = packing_plan(np.asarray(lens, np.int32), S).to(DEV, non_blocking=False) if packed else None
        assert self.plan is None or self.plan.packed
        T = self.plan.rows if packed else B * S
        d = {k: v.to(DEV) for k, v in tb.items()}
        lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
        self.keep = [d, lens_d] + [None if t is None else t.to(DEV).contiguous() for t in (ids, tt, pid, xe, dy)]
        ids_d, tt_d, pid_d, xe_d, dy_d = self.keep[2:]
        ptr = lambda t: None if t is None else t.data_ptr()
        self.out = torch.full((T, E), 7.0, dtype=torch.bfloat16, device=DEV)
        self.dx = torch.full((T, E), 7.0, device=DEV)
        self.part = torch.full((nblocks, 2 * E), 7.0, device=DEV)
        self.dword, self.dpos = torch.full((V, E), 7.0, device=DEV), torch.full((P, E), 7.0, device=DEV)
        self.dtype_rows = torch.full((NTY, E), 7.0, device=DEV)
        self.die = torch.full((B, S, E), 7.0, device=DEV) if want_die else None
        nfl = int(L.plb_embed_inputs_part_floats(B * S, P, NTY, E))
        assert nfl == ((B * S + 511) // 512) * (P + NTY) * E
        self.chunk_part = torch.full((nfl,), 7.0, device=DEV)
        p = _lib.PlbEmbed()
        p.ids, p.T, p.S, p.E, p.V = ptr(ids_d), T, S, E, V
        p.word, p.pos, p.type0, p.gamma, p.beta = (d[k].data_ptr() for k in ("word", "pos", "type", "gamma", "beta"))
        p.eps, p.out, p.ldo = 1e-12, self.out.data_ptr(), E
        p.dout, p.lddo, p.dx, p.dword, p.dpos = dy_d.data_ptr(), E, self.dx.data_ptr(), self.dword.data_ptr(), self.dpos.data_ptr()
        p.partials, p.nblocks = self.part.data_ptr(), nblocks
        p.lengths, p.B = ptr(lens_d), B
        if packed:
            p.row_start = self.plan.row_start.data_ptr()
        self.plain = tt is None and pid is None and xe is None
        if self.plain:
            assert L.plb_launch_embed_fwd(C.byref(p), stream()) == 0
            assert L.plb_launch_embed_bwd(C.byref(p), stream()) == 0
            assert L.plb_launch_embed_scatter(C.byref(p), P, stream()) == 0
        else:
            x = _lib.PlbEmbedIn()
            x.base = C.addressof(p)
            x.token_type_ids, x.position_ids, x.inputs_embeds, x.NTY, x.P = ptr(tt_d), ptr(pid_d), ptr(xe_d), NTY, P
            x.dtype_rows, x.d_inputs_embeds, x.chunk_part = self.dtype_rows.data_ptr(), ptr(self.die), self.chunk_part.data_ptr()
            assert L.plb_launch_embed_inputs_fwd(C.byref(x), stream()) == 0
            assert L.plb_launch_embed_inputs_bwd(C.byref(x), stream()) == 0
            assert L.plb_launch_embed_inputs_scatter(C.byref(x), stream()) == 0
        torch.cuda.synchronize()
        # where token (b, s) sits on the row axis, and which tokens the call counts (packed: the valid ones)
        bs = torch.arange(B * S).view(B, S)
        valid = torch.ones(B, S, dtype=torch.bool) if lens is None else torch.arange(S)[None, :] < torch.tensor(lens)[:, None]
        self.valid = valid
        self.rows = (self.plan.row_start.cpu()[:B, None].long() + torch.arange(S)[None, :]) if packed else bs
        self.counted = valid if packed else torch.ones(B, S, dtype=torch.bool)


@pytest.mark.parametrize("source", ["ids", "embeds"])
@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("E", [64, 128, 256])
def test_forward_and_dx_against_float64(E, layout, source):
    """The bounds of test_gpu_rowops.py::test_embeddings_forward_backward_scatter for the same quantities."""
    shape, packed = K_SHAPE, layout == "packed"
    B, S, lens = shape
    tb = _tables(E, 10 + E)
    ids, tt, pid, xe, g = _batch(E, shape, "random", 20 + E)
    T = packing_plan(np.asarray(lens, np.int32), S).rows if packed else B * S
    dy = (0.3 + torch.randn(T, E, generator=g)).to(torch.bfloat16)
    r = Run(E, shape, packed, tb, ids if source == "ids" else None, tt, pid, xe if source == "embeds" else None, dy)
    sel = r.counted
    rows = r.rows[sel]
    g64, b64 = tb["gamma"].double().requires_grad_(), tb["beta"].double().requires_grad_()
    base = tb["word"].double()[ids[sel]] if source == "ids" else xe.double()[sel]
    x = (base + tb["type"].double()[tt[sel]] + tb["pos"].double()[pid[sel]]).detach().requires_grad_()
    y = torch.nn.functional.layer_norm(x, (E,), g64, b64, eps=1e-12)
    y.backward(dy.double()[rows])
    got, yd = r.out.cpu().double()[rows], y.detach()
    assert bool(((got - yd).abs() <= 2.0 ** -8 * yd.abs() + 1e-5 * float(yd.abs().max())).all())
    dxg = r.dx.cpu().double()
    assert torch.allclose(dxg[rows], x.grad, rtol=1e-5, atol=1e-5 * float(x.grad.abs().max()))
    ps = r.part.cpu().double().sum(0)
    for got_v, want_v in ((ps[:E], g64.grad), (ps[E:], b64.grad)):
        assert float((got_v - want_v).abs().max()) <= 1e-5 * float(want_v.abs().max())
    if packed:   # rows that hold no token: zeros from the forward and the backward
        free = torch.ones(T, dtype=torch.bool)
        free[rows] = False
        assert free.any() and not bool(r.out.cpu()[free].view(torch.int16).any()) and not bool(r.dx.cpu()[free].view(torch.int32).any())


@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("E", [64, 128, 256])
def test_explicit_defaults_are_bit_equal_to_the_plain_launches(E, layout):
    shape, packed = K_SHAPE, layout == "packed"
    B, S, lens = shape
    tb = _tables(E, 30 + E)
    ids, _, _, _, g = _batch(E, shape, "random", 40 + E)
    T = packing_plan(np.asarray(lens, np.int32), S).rows if packed else B * S
    dy = (0.3 + torch.randn(T, E, generator=g)).to(torch.bfloat16)
    plain = Run(E, shape, packed, tb, ids, None, None, None, dy, want_die=False)
    tt0, pid0 = torch.zeros(B, S, dtype=torch.int64), torch.arange(S).expand(B, S).contiguous()
    r = Run(E, shape, packed, tb, ids, tt0, pid0, None, dy)
    assert torch.equal(r.out.view(torch.int16), plain.out.view(torch.int16))
    assert torch.equal(r.dx.view(torch.int32), plain.dx.view(torch.int32))
    assert torch.equal(r.part.view(torch.int32), plain.part.view(torch.int32))
    assert torch.equal(r.dword.view(torch.int32), plain.dword.view(torch.int32))   # (the same kernel sums the word rows)


def _check_sum(got, keys, terms, nrows, what):
    """got[row] against the float64 sum of `terms` (fp32 dx rows) by key, element by element: n * 2^-24 * sum|terms|."""
    E = terms.shape[1]
    want = torch.zeros(nrows, E, dtype=torch.float64).index_add_(0, keys, terms)
    mag = torch.zeros(nrows, E, dtype=torch.float64).index_add_(0, keys, terms.abs())
    n = torch.zeros(nrows, dtype=torch.float64).index_add_(0, keys, torch.ones(len(keys), dtype=torch.float64))
    err = (got.double() - want).abs()
    bound = n[:, None] * 2.0 ** -24 * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: largest error / bound {worst:.3f}, longest list {int(n.max())}, rows without a token {int((n == 0).sum())}")
    assert bool((err <= bound).all()), (what, worst)
    assert not bool(got[n == 0].view(torch.int32).any()), what          # nobody's rows: exactly +0.0
    assert bool((got[n == 1].double() == want[n == 1]).all()), what     # one term: exact
    return n


@pytest.mark.parametrize("case", ["padded-random", "packed-random", "padded-one", "packed-one", "padded-unused", "packed-unused",
                                  "chunks"])
@pytest.mark.parametrize("E", [64, 128, 256])
def test_table_sums_reproducibility_and_d_inputs_embeds(E, case):
    layout, _, pattern = case.partition("-")
    shape, packed = (CHUNKS, False) if case == "chunks" else (K_SHAPE, layout == "packed")
    B, S, lens = shape
    tb = _tables(E, 50 + E)
    ids, tt, pid, xe, g = _batch(E, shape, pattern, 60 + E)
    if case == "chunks":   # three full 512-token chunks on ONE type row: three partial rows, added in chunk order
        tt[:] = 2
    T = packing_plan(np.asarray(lens, np.int32), S).rows if packed else B * S
    dy = (0.3 + torch.randn(T, E, generator=g)).to(torch.bfloat16)
    r = Run(E, shape, packed, tb, ids, tt, pid, None, dy)
    sel = r.counted
    terms = r.dx.cpu().double()[r.rows[sel]]
    nw = _check_sum(r.dword.cpu(), ids[sel], terms * (ids[sel] != 0)[:, None], V, "word")
    assert not bool(r.dword[0].view(torch.int32).any()) and nw[0] > 0          # the padding row: tokens, and no gradient
    n_pos = _check_sum(r.dpos.cpu(), pid[sel], terms, P, "position")
    n_ty = _check_sum(r.dtype_rows.cpu(), tt[sel], terms, NTY, "token type")
    if pattern == "one":
        assert int((n_pos > 0).sum()) == 1 and int((n_ty > 0).sum()) == 1 and n_ty[1] == int(sel.sum()) > 512
    if pattern == "unused":
        assert n_ty[1] == 0 and not bool((n_pos[100:] > 0).any())
    if case == "chunks":
        assert n_ty[2] == 3 * 512
    # d_inputs_embeds: the dx rows in the padded layout, bit for bit; exactly zero at pad positions
    die = r.die.cpu()
    assert torch.equal(die[r.valid].view(torch.int32), r.dx.cpu()[r.rows[r.valid]].view(torch.int32))
    if lens is not None:
        assert not bool(die[~r.valid].view(torch.int32).any()) and bool((~r.valid).any())
    # a second run: bit-equal
    r2 = Run(E, shape, packed, tb, ids, tt, pid, None, dy)
    for a, b in ((r.dword, r2.dword), (r.dpos, r2.dpos), (r.dtype_rows, r2.dtype_rows), (r.dx, r2.dx), (r.die, r2.die)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_inputs_embeds_zeroes_the_word_table_and_types_alone_keep_the_strided_position_sum(layout):
    """inputs_embeds: the word table's gradient is written as zeros. token_type_ids without position_ids: the position rows
    are summed by the plain launch's kernel (a strided sum over the batch), the type rows sum their own tokens."""
    E, shape, packed = 128, K_SHAPE, layout == "packed"
    B, S, lens = shape
    tb = _tables(E, 70)
    ids, tt, pid, xe, g = _batch(E, shape, "random", 80)
    T = packing_plan(np.asarray(lens, np.int32), S).rows if packed else B * S
    dy = (0.3 + torch.randn(T, E, generator=g)).to(torch.bfloat16)
    r = Run(E, shape, packed, tb, None, None, pid, xe, dy)
    assert not bool(r.dword.view(torch.int32).any())
    terms = r.dx.cpu().double()[r.rows[r.counted]]
    _check_sum(r.dpos.cpu(), pid[r.counted], terms, P, "position (inputs_embeds)")
    _check_sum(r.dtype_rows.cpu(), torch.zeros(int(r.counted.sum()), dtype=torch.int64), terms, NTY, "token type (row 0 of all)")
    r = Run(E, shape, packed, tb, ids, tt, None, None, dy)
    s_of = torch.arange(S).expand(B, S)
    terms = r.dx.cpu().double()[r.rows[r.counted]]
    _check_sum(r.dpos.cpu(), s_of[r.counted], terms, P, "position (strided)")
    _check_sum(r.dtype_rows.cpu(), tt[r.counted], terms, NTY, "token type")


def test_launchers_refuse_bad_arguments():
    L = _lib.lib()
    p, x = _lib.PlbEmbed(), _lib.PlbEmbedIn()
    for fn in (L.plb_launch_embed_inputs_fwd, L.plb_launch_embed_inputs_bwd, L.plb_launch_embed_inputs_scatter):
        assert fn(C.byref(x), stream()) != 0            # no base
        x.base = C.addressof(p)
        assert fn(C.byref(x), stream()) != 0            # no shape, neither ids nor inputs_embeds
        x.base = None
