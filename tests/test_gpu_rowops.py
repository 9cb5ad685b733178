"""Row kernels of the step at kernel level (-m gpu; csrc/embed.hip, reduce.hip, loss_rows.hip, operand_images.hip), each
launched through the C ABI and compared with a float64 restatement of the operation (or bit for bit, where the kernel only moves or rounds values):
 * the masked-phoneme cross-entropy (ce_prepare -> ce_fwd_bwd -> sum_rows), the loss bench.py times;
 * LayerNorm_E of the embedding sum, forward and backward, the dgamma / dbeta partials and the scatter into the tables;
 * the pooler, as a launch and through an engine;
 * the copies and casts: gather / scatter of rows, transposes, bf16 casts, column sums finished by copy_cols.
Bounds: a bf16 store is allowed one bf16 rounding (2^-8 relative) plus the fp32 arithmetic before it; a sum in fp32 is
allowed 1e-5 of the sum of its terms' magnitudes (the standard bound for recursive summation: the kernels add at most a
few thousand terms per chain)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import ptr_array, stream
import plbert_amd
from plbert_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24   # unit roundoff of fp32


# -------------------------------------------------------------------------------------------- masked cross-entropy
def _csr(counts, lens, S, g):
    flat, off = [], [0]
    for n, ln in zip(counts, lens):
        flat += sorted(g.choice(ln, size=n, replace=False).tolist())
        off.append(off[-1] + n)
    return np.array(off, np.int32), np.array(flat, np.int32)


def _ce_case(B, S, V, counts, seed):
    g = np.random.default_rng(seed)
    lens = [S] * B
    off, flat = _csr(counts, lens, S, g)
    labels = g.integers(0, V, size=(B, S)).astype(np.int64)
    n = int(off[-1])
    # targets 0 and V-1 appear
    if n >= 2:
        b0 = int(np.searchsorted(off, 0, side="right") - 1)
        labels[b0, flat[0]] = 0
        b1 = int(np.searchsorted(off, n - 1, side="right") - 1)
        labels[b1, flat[n - 1]] = V - 1
    return off, flat, labels, n


def _run_ce(off, flat, labels, B, S, V, logits_rows, npad, ldd=256):
    L = _lib.lib()
    n = int(off[-1])
    d_off = torch.from_numpy(off).to(DEV)
    d_flat = torch.from_numpy(flat if len(flat) else np.zeros(1, np.int32)).to(DEV)
    d_lab = torch.from_numpy(labels).to(DEV)
    rows = torch.full((max(n, 1),), -1, dtype=torch.int32, device=DEV)
    tgt = torch.full((max(n, 1),), -1, dtype=torch.int32, device=DEV)
    w = torch.full((max(n, 1),), -1.0, device=DEV)
    assert L.plb_launch_ce_prepare(d_off.data_ptr(), d_flat.data_ptr(), d_lab.data_ptr(), B, S, rows.data_ptr(),
                                   tgt.data_ptr(), w.data_ptr(), stream()) == 0
    ldl = V + 5
    logits = torch.full((npad, ldl), 1e4, dtype=torch.float32)   # columns >= V must not count
    logits[:n, :V] = logits_rows
    logits = logits.to(DEV)
    loss_rows = torch.full((npad,), 7.0, device=DEV)
    dlog = torch.full((npad, ldd), 7.0, dtype=torch.bfloat16, device=DEV)
    out = torch.full((1,), 7.0, device=DEV)
    assert L.plb_launch_ce_fwd_bwd(logits.data_ptr(), ldl, V, tgt.data_ptr(), w.data_ptr(), n, npad, loss_rows.data_ptr(),
                                   dlog.data_ptr(), ldd, stream()) == 0
    assert L.plb_launch_sum_rows(loss_rows.data_ptr(), n, out.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    return rows.cpu(), tgt.cpu(), w.cpu(), loss_rows.cpu(), dlog.cpu(), float(out.item())


@pytest.mark.parametrize("B,S,V,counts", [(6, 64, 188, [5, 0, 17, 1, 0, 40]), (4, 96, 256, [0, 0, 7, 0]),
                                          (3, 33, 10, [33, 2, 9]), (8, 512, 188, [77, 76, 0, 80, 12, 64, 0, 3])])
def test_masked_cross_entropy(B, S, V, counts):
    g = np.random.default_rng(B * 1000 + V)
    off, flat, labels, n = _ce_case(B, S, V, counts, seed=V + B)
    z = torch.from_numpy(g.uniform(-80, 80, size=(n, V)).astype(np.float32))   # exp underflows after the max shift
    z[1::3] = torch.from_numpy(g.normal(0, 2, size=z[1::3].shape).astype(np.float32))
    z[0] = 3.0                                                                    # a row of equal logits
    npad = n + 7
    rows, tgt, w, loss_rows, dlog, total = _run_ce(off, flat, labels, B, S, V, z, npad)
    # ce_prepare: rows / targets / weights, exactly
    sample = np.repeat(np.arange(B), np.diff(off))
    count = int((np.diff(off) > 0).sum())
    nb = np.diff(off)[sample]
    assert torch.equal(rows[:n], torch.from_numpy((sample * S + flat).astype(np.int32)))
    assert torch.equal(tgt[:n], torch.from_numpy(labels[sample, flat].astype(np.int32)))
    w_want = np.float32(1.0) / (nb.astype(np.float32) * np.float32(count))
    assert np.array_equal(w[:n].numpy(), w_want)
    # the loss: calculate_phoneme_loss in float64 — mean over each sample's masked rows, then over the samples that have any
    zd = z.double()
    t = torch.from_numpy(labels[sample, flat])
    lse = torch.logsumexp(zd, 1)
    ce = lse - zd[torch.arange(n), t]
    want_total = sum(float(ce[torch.from_numpy(sample == b)].mean()) for b in range(B) if counts[b]) / count
    wd = torch.from_numpy(w_want).double()
    want_rows = wd * ce
    # fp32 evaluation of w * (max + log(sum) - z_t): a few roundings of operands of magnitude |lse|, |z_t|
    tol_rows = 1e-6 * want_rows.abs() + 1e-6 * wd * (lse.abs() + zd[torch.arange(n), t].abs() + 1)
    err = (loss_rows[:n].double() - want_rows).abs()
    assert bool((err <= tol_rows).all()), float((err / tol_rows).max())
    assert bool((loss_rows[n:] == 7.0).all())                                      # padding rows carry no loss row
    depth = -(-n // 256) + 9
    tol_total = 1e-6 * abs(want_total) + float(tol_rows.sum()) + depth * U32 * float(loss_rows[:n].double().abs().sum())
    assert abs(total - want_total) <= tol_total, (total, want_total, tol_total)
    # the gradient: w * (softmax - onehot), one bf16 rounding of an fp32 value
    r = wd[:, None] * (torch.softmax(zd, 1) - torch.nn.functional.one_hot(t, V).double())
    got = dlog[:n, :V].double()
    assert bool(((got - r).abs() <= 2.0 ** -8 * r.abs() + 4e-6 * wd[:, None]).all())
    assert bool((dlog[:n, V:] == 0).all()) and bool((dlog[n:] == 0).all())       # padding columns and rows: exact zeros
    # the equal-logits row: 1 / V each
    assert abs(float(loss_rows[0]) - float(wd[0]) * np.log(V)) <= 1e-6 * float(wd[0]) * (np.log(V) + 7)


@pytest.mark.parametrize("n", [0, 1, 257, 5000])
def test_sum_rows(n):
    L = _lib.lib()
    g = torch.Generator().manual_seed(n)
    x = (torch.rand(max(n, 1), generator=g) - 0.3) * 10
    xd = x.to(DEV)
    outs = []
    for _ in range(3):
        out = torch.full((1,), 7.0, device=DEV)
        assert L.plb_launch_sum_rows(xd.data_ptr(), n, out.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert all(torch.equal(o, outs[0]) for o in outs)                  # one block, fixed order
    want = float(x[:n].double().sum())
    depth = -(-n // 256) + 9                                           # per-thread chain, wave butterfly, 4 wave sums
    assert abs(float(outs[0]) - want) <= depth * U32 * float(x[:n].double().abs().sum()), (float(outs[0]), want)
    if n == 0:
        assert float(outs[0]) == 0.0


def test_ce_refuses_beyond_its_width():
    L = _lib.lib()
    buf = torch.zeros(1024, device=DEV)
    assert L.plb_launch_ce_fwd_bwd(buf.data_ptr(), 300, 257, buf.data_ptr(), buf.data_ptr(), 1, 1, buf.data_ptr(),
                                   buf.data_ptr(), 256, stream()) != 0
    assert L.plb_launch_ce_fwd_bwd(buf.data_ptr(), 256, 188, buf.data_ptr(), buf.data_ptr(), 1, 1, buf.data_ptr(),
                                   buf.data_ptr(), 258, stream()) != 0


# ------------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("E", [64, 128, 256])
@pytest.mark.parametrize("nblocks", [1, 64])
def test_embeddings_forward_backward_scatter(E, nblocks):
    L = _lib.lib()
    g = torch.Generator().manual_seed(E + nblocks)
    V, S, P, T = 188, 512, 520, 9003                  # T > 2048 blocks x 4 waves, not a multiple of 4; P > S
    word = torch.randn(V, E, generator=g)
    pos = torch.randn(P, E, generator=g) * 0.5
    type0 = torch.randn(E, generator=g) * 0.3
    gamma = 1 + 0.3 * torch.randn(E, generator=g)
    beta = 0.2 * torch.randn(E, generator=g)
    ids = torch.randint(0, V, (T,), generator=g)
    hot = torch.rand(T, generator=g)
    ids[hot < 0.35] = 3                               # a few ids own most of the tokens
    ids[(hot >= 0.35) & (hot < 0.55)] = 4
    ids[(hot >= 0.55) & (hot < 0.6)] = 0              # the padding id
    dy = (0.3 + torch.randn(T, E, generator=g)).to(torch.bfloat16)
    d = {k: v.to(DEV) for k, v in dict(word=word, pos=pos, type0=type0, gamma=gamma, beta=beta, ids=ids, dy=dy).items()}
    ldo = E + 8
    out = torch.full((T, ldo), 7.0, dtype=torch.bfloat16, device=DEV)
    dx = torch.full((T, E), 7.0, device=DEV)
    part = torch.full((nblocks, 2 * E), 7.0, device=DEV)
    dword = torch.full((V, E), 7.0, device=DEV)
    dpos = torch.full((P, E), 7.0, device=DEV)
    p = _lib.PlbEmbed()
    p.ids, p.T, p.S, p.E, p.V = d["ids"].data_ptr(), T, S, E, V
    p.word, p.pos, p.type0, p.gamma, p.beta = (d[k].data_ptr() for k in ("word", "pos", "type0", "gamma", "beta"))
    p.eps, p.out, p.ldo = 1e-12, out.data_ptr(), ldo
    p.dout, p.lddo, p.dx, p.dword, p.dpos = d["dy"].data_ptr(), E, dx.data_ptr(), dword.data_ptr(), dpos.data_ptr()
    p.partials, p.nblocks = part.data_ptr(), nblocks
    assert L.plb_launch_embed_fwd(C.byref(p), stream()) == 0
    assert L.plb_launch_embed_bwd(C.byref(p), stream()) == 0
    assert L.plb_launch_embed_scatter(C.byref(p), P, stream()) == 0
    torch.cuda.synchronize()
    # float64 autograd of LayerNorm_E(word[ids] + type0 + pos[t % S])
    w64, p64, t64 = word.double().requires_grad_(), pos.double(), type0.double()
    g64, b64 = gamma.double().requires_grad_(), beta.double().requires_grad_()
    x = (w64[ids] + t64 + p64[torch.arange(T) % S]).detach().requires_grad_()
    y = torch.nn.functional.layer_norm(x, (E,), g64, b64, eps=1e-12)
    y.backward(dy.double())
    got = out.cpu()
    ymax = float(y.detach().abs().max())
    assert bool(((got[:, :E].double() - y.detach()).abs() <= 2.0 ** -8 * y.detach().abs() + 1e-5 * ymax).all())
    assert bool((got[:, E:] == 7.0).all())                                       # columns past E untouched
    dxg = dx.cpu().double()
    assert torch.allclose(dxg, x.grad, rtol=1e-5, atol=1e-5 * float(x.grad.abs().max()))
    ps = part.cpu().double().sum(0)
    for got_v, want_v in ((ps[:E], g64.grad), (ps[E:], b64.grad)):
        assert float((got_v - want_v).abs().max()) <= 1e-5 * float(want_v.abs().max()), float((got_v - want_v).abs().max())
    # scatter of the kernel's own dx into the tables: index_add in float64, row 0 of the word table and positions >= S zero
    want_w = torch.zeros(V, E, dtype=torch.float64).index_add_(0, ids, dxg)
    mag_w = torch.zeros(V, E, dtype=torch.float64).index_add_(0, ids, dxg.abs())
    want_w[0] = 0
    mag_w[0] = 0
    want_p = torch.zeros(P, E, dtype=torch.float64).index_add_(0, torch.arange(T) % S, dxg)
    mag_p = torch.zeros(P, E, dtype=torch.float64).index_add_(0, torch.arange(T) % S, dxg.abs())
    gw, gp = dword.cpu().double(), dpos.cpu().double()
    assert bool(((gw - want_w).abs() <= 1e-5 * mag_w).all())
    assert bool((gp - want_p).abs().le(1e-5 * mag_p).all())
    assert bool((gw[0] == 0).all()) and bool((gp[S:] == 0).all())


# ----------------------------------------------------------------------------------------------------------- pooler
@pytest.mark.parametrize("H", [128, 768, 1024])
@pytest.mark.parametrize("B,S", [(1, 1), (3, 512)])
def test_pooler_launch(H, B, S):
    L = _lib.lib()
    g = torch.Generator().manual_seed(H + B + S)
    hidden = torch.randn(B, S, H, generator=g)
    W = torch.randn(H, H, generator=g) * H ** -0.5
    b = torch.randn(H, generator=g) * 0.2
    hd, Wd, bd = hidden.to(DEV), W.to(DEV), b.to(DEV)
    out = torch.full((B + 1, H), 7.0, device=DEV)
    assert L.plb_launch_pooler(hd.data_ptr(), B, S, H, Wd.data_ptr(), bd.data_ptr(), out.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    want = torch.tanh(hidden[:, 0].double() @ W.double().T + b.double())
    assert float((out[:B].cpu().double() - want).abs().max()) <= 1e-5
    assert bool((out[B:] == 7.0).all())


@pytest.mark.parametrize("H,NH", [(128, 2), (768, 12), (1024, 16)])
def test_pooler_through_an_engine(H, NH):
    from plbert_amd.engine import HipEngine
    cfg = plbert_amd.AlbertConfig(vocab_size=188, embedding_size=128, hidden_size=H, num_attention_heads=NH,
                                  intermediate_size=2 * H, num_hidden_layers=1)
    sd = plbert_amd.deterministic_state_dict(cfg, 188, seed=3)
    W = torch.from_numpy(np.asarray(sd["encoder.pooler.weight"])).double()
    b = torch.from_numpy(np.asarray(sd["encoder.pooler.bias"])).double()
    eng = HipEngine(cfg, 188, 0, max_batch=3, max_seq=512, train=False)
    eng.load_state_dict(sd)
    for B, S in ((1, 1), (3, 512)):
        hidden = torch.randn(B, S, H, generator=torch.Generator().manual_seed(B)) * 2
        got = eng.pooler(hidden.to(DEV))
        torch.cuda.synchronize()
        want = torch.tanh(hidden[:, 0].double() @ W.T + b)
        assert float((got.cpu().double() - want).abs().max()) <= 1e-5


# ----------------------------------------------------------------------------------------------- copies and casts
def test_gather_and_scatter_rows():
    L = _lib.lib()
    g = torch.Generator().manual_seed(11)
    T, H, lds, ldd, n, npad = 300, 768, 776, 784, 57, 64
    src = torch.randn(T, lds, generator=g).to(torch.bfloat16)
    rows = torch.randperm(T, generator=g)[:n].to(torch.int32)          # arbitrary order
    sd, rd = src.to(DEV), rows.to(DEV)
    dst = torch.full((npad, ldd), 7.0, dtype=torch.bfloat16, device=DEV)
    assert L.plb_launch_gather_rows(sd.data_ptr(), lds, rd.data_ptr(), n, npad, H, dst.data_ptr(), ldd, stream()) == 0
    torch.cuda.synchronize()
    d = dst.cpu()
    assert torch.equal(d[:n, :H], src[rows.long(), :H])
    assert bool((d[n:, :H] == 0).all()) and bool((d[:, H:] == 7.0).all())
    # scatter: compact rows back to distinct token rows; untouched rows keep their sentinel
    comp = torch.randn(n, lds, generator=g).to(torch.bfloat16)
    out = torch.full((T, ldd), 7.0, dtype=torch.bfloat16, device=DEV)
    cd = comp.to(DEV)
    assert L.plb_launch_scatter_rows(cd.data_ptr(), lds, rd.data_ptr(), n, H, out.data_ptr(), ldd, stream()) == 0
    torch.cuda.synchronize()
    o = out.cpu()
    want = torch.full((T, ldd), 7.0, dtype=torch.bfloat16)
    want[rows.long(), :H] = comp[:, :H]
    assert torch.equal(o, want)


def test_transpose_cast_single_and_multi():
    L = _lib.lib()
    g = torch.Generator().manual_seed(12)
    shapes = [(33, 1, 33), (1, 1, 8), (768, 2304, 768), (45, 70, 64), (32, 32, 40), (100, 3, 100), (7, 129, 7), (64, 33, 72)]
    srcs = [torch.randn(R, Cc, generator=g) * 3 for R, Cc, _ in shapes]
    for (R, Cc, ldd), s in zip(shapes[:3] + shapes[3:4], srcs[:3] + srcs[3:4]):
        dst = torch.full((Cc, ldd), 7.0, dtype=torch.bfloat16, device=DEV)
        sd = s.to(DEV)
        assert L.plb_launch_transpose_cast(sd.data_ptr(), R, Cc, dst.data_ptr(), ldd, stream()) == 0
        torch.cuda.synchronize()
        d = dst.cpu()
        assert torch.equal(d[:, :R], s.t().to(torch.bfloat16)) and bool((d[:, R:] == 7.0).all())
    sds = [s.to(DEV) for s in srcs]
    dsts = [torch.full((Cc, ldd), 7.0, dtype=torch.bfloat16, device=DEV) for R, Cc, ldd in shapes]
    n = len(shapes)
    ints = lambda v: (C.c_int * n)(*v)  # noqa: E731
    assert L.plb_launch_transpose_cast_multi(n, ptr_array(sds), ints([s[0] for s in shapes]), ints([s[1] for s in shapes]),
                                             ptr_array(dsts), ints([s[2] for s in shapes]), stream()) == 0
    torch.cuda.synchronize()
    for (R, Cc, ldd), s, dst in zip(shapes, srcs, dsts):
        d = dst.cpu()
        assert torch.equal(d[:, :R], s.t().to(torch.bfloat16)), (R, Cc)
        assert bool((d[:, R:] == 7.0).all()), (R, Cc)
    bad = ints([s[2] - 1 if i == 2 else s[2] for i, s in enumerate(shapes)])   # ldd < R: refused on the host
    assert L.plb_launch_transpose_cast_multi(n, ptr_array(sds), ints([s[0] for s in shapes]), ints([s[1] for s in shapes]),
                                             ptr_array(dsts), bad, stream()) != 0


def test_cast_bf16_rounding():
    L = _lib.lib()
    g = torch.Generator().manual_seed(13)
    b = (torch.randn(4000, generator=g) * 10.0 ** torch.randint(-30, 30, (4000,), generator=g)).to(torch.bfloat16)
    bits = b.view(torch.int16).int()
    nxt = (bits + 1).to(torch.int16).view(torch.bfloat16)               # the next bf16 away from zero
    mid = (b.double() + nxt.double()) / 2                               # 9 significant bits: exact in fp32
    mid32 = mid.float()
    fin = torch.isfinite(mid32) & torch.isfinite(nxt.float())
    mid32 = mid32[fin]
    up = torch.nextafter(mid32, torch.full_like(mid32, float("inf")))
    dn = torch.nextafter(mid32, torch.full_like(mid32, -float("inf")))
    special = torch.tensor([float("inf"), -float("inf"), 0.0, -0.0, 1e-45, -1e-45, 1e-40, 2.0 ** -126, 3.3895e38, -3.3895e38,
                            3.4e38], dtype=torch.float32)
    x = torch.cat([torch.randn(5000, generator=g) * 100, mid32, up, dn, special])
    xd = x.to(DEV)
    out = torch.full((x.numel() + 16,), 7.0, dtype=torch.bfloat16, device=DEV)
    assert L.plb_launch_cast_bf16(xd.data_ptr(), out.data_ptr(), x.numel(), stream()) == 0
    torch.cuda.synchronize()
    o = out.cpu()
    assert torch.equal(o[:x.numel()].view(torch.int16), x.to(torch.bfloat16).view(torch.int16))
    assert bool((o[x.numel():] == 7.0).all())


def test_bf16_to_f32_strided():
    L = _lib.lib()
    g = torch.Generator().manual_seed(14)
    R, Cc, lds, ldd = 130, 77, 96, 80
    src = torch.randn(R, lds, generator=g).to(torch.bfloat16)
    sd = src.to(DEV)
    dst = torch.full((R, ldd), 7.0, device=DEV)
    assert L.plb_launch_bf16_to_f32(sd.data_ptr(), lds, dst.data_ptr(), ldd, R, Cc, stream()) == 0
    torch.cuda.synchronize()
    d = dst.cpu()
    assert torch.equal(d[:, :Cc], src[:, :Cc].float()) and bool((d[:, Cc:] == 7.0).all())


@pytest.mark.parametrize("is_bf16", [1, 0])
def test_colsum_then_copy_cols(is_bf16):
    L = _lib.lib()
    g = torch.Generator().manual_seed(15 + is_bf16)
    R, N, ld, Nout, nsplit, col0, Nout2 = 1001, 264, 272, 200, 7, 200, 64
    X = 0.5 + torch.randn(R, ld, generator=g)
    X = X.to(torch.bfloat16) if is_bf16 else X
    Xd = X.to(DEV)
    scratch = torch.zeros(nsplit, N, device=DEV)
    col = X[:, :N].double()
    want, mag = col.sum(0), col.abs().sum(0)
    for accumulate in (0, 1):
        out = torch.full((N,), 7.0, device=DEV)
        base = out.cpu().double()
        assert L.plb_launch_colsum(Xd.data_ptr(), is_bf16, R, N, ld, out.data_ptr(), Nout, accumulate, scratch.data_ptr(),
                                   nsplit, stream()) == 0
        out2 = torch.full((Nout2 + 4,), 7.0, device=DEV)
        assert L.plb_launch_copy_cols(scratch.data_ptr(), nsplit, N, col0, Nout2, out2.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        o, o2 = out.cpu().double(), out2.cpu().double()
        exp = want[:Nout] + (base[:Nout] if accumulate else 0)
        assert bool(((o[:Nout] - exp).abs() <= 1e-5 * (mag[:Nout] + base[:Nout].abs() * accumulate)).all())
        assert bool((o[Nout:] == 7.0).all())                                      # only Nout sums are written
        assert bool(((o2[:Nout2] - want[col0:col0 + Nout2]).abs() <= 1e-5 * mag[col0:col0 + Nout2]).all())
        assert bool((o2[Nout2:] == 7.0).all())
    assert L.plb_launch_copy_cols(scratch.data_ptr(), nsplit, N, col0, N - col0 + 1, out2.data_ptr(), stream()) != 0
