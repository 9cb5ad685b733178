"""Token-packed execution of ragged batches (include/plbert.h: PlbPacking) on the GPU: the packed kernels against the padded
launches on the same data (bit-equal on valid rows: a sample's 128-row slots hold the tiles of the padded call), the
packed engine path against the reference fixtures, the numpy oracle and the padded path, its independence of what an
earlier call left in the workspace, graph capture, and the calls that run padded although they were given a plan."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_cfg, load_golden
from gpu_util import attn_args, rel_l2, stream
from oracle import albert_np as onp
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import HipEngine, packing_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY_BIAS = "encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.key.bias"
QUERY_BIAS = KEY_BIAS.replace("key", "query")


def randbf(r, c, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(r, c, generator=g) * scale).to(torch.bfloat16).to(DEV)


def _plan(lengths, S):
    plan = packing_plan(lengths, S).to(DEV, non_blocking=False)
    assert plan.packed
    return plan


def _row_index(plan):
    """(packed row, padded row) of every valid token, and the mask of packed rows that hold no token."""
    pr, dr = [], []
    for b in range(plan.B):
        n = int(min(max(plan.lengths[b], 1), plan.S))
        pr.append(torch.arange(n) + int(plan.row_start_host[b]))
        dr.append(torch.arange(n) + b * plan.S)
    pr, dr = torch.cat(pr).to(DEV), torch.cat(dr).to(DEV)
    hole = torch.ones(plan.rows, dtype=torch.bool, device=DEV)
    hole[pr] = False
    return pr, dr, hole


def _pack_rows(x, plan, fill=0.0):
    """[B*S, C] -> [rows, C]: valid tokens at their packed rows, ``fill`` elsewhere."""
    pr, dr, _ = _row_index(plan)
    out = torch.full((plan.rows, x.shape[1]), fill, dtype=x.dtype, device=x.device)
    out[pr] = x[dr]
    return out


LENS = [512, 449, 300, 130, 65, 1]
# 24 samples x 12 heads: with the hybrid policy (form 2) the first 21 samples (one round of 252 items) take the single-kernel
# form and the last 3 the two kernels (attn.hip: attn_samples) — both kinds of sample ragged
LENS_HYBRID = [512, 500, 449, 385, 384, 300, 257, 256, 200, 130, 129, 128, 127, 65, 64, 63, 33, 2, 1, 512, 74, 512, 300, 1]


@pytest.mark.parametrize("form,lens,NH", [(0, LENS, 4), (1, LENS, 4), (2, LENS_HYBRID, 12)])
def test_packed_attention_is_bit_equal_to_the_padded_launch_on_valid_rows(form, lens, NH):
    """Forward and the backward forms (0: dQ + dK/dV kernels, 1: the single-kernel form, 2: the per-shape policy with the
    batch split by sample between the two). Rows of a slot behind the sample's length hold an arbitrary value (0.5) in the
    packed input: they are masked keys and unread queries, as the padded rows of the padded call. Tiles past a sample's
    slot are not touched (sentinel), their bias-gradient partial rows are zeros."""
    L = _lib.lib()
    LENS = lens
    B, S = len(LENS), 512
    H, QT = NH * 64, 4
    lengths = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    plan = _plan(LENS, S)
    pr, dr, hole = _row_index(plan)
    qkv = randbf(B * S, 3 * H, seed=5)
    dctx = randbf(B * S, H, seed=6)
    qmask = (torch.arange(S, device=DEV)[None, :] < lengths[:, None]).reshape(B * S, 1)
    dctx = dctx * qmask.to(dctx.dtype)
    L.plb_set_attn_bwd_fused(form)
    try:
        out = {}
        for packed in (False, True):
            q = _pack_rows(qkv, plan, 0.5) if packed else qkv
            d = _pack_rows(dctx, plan) if packed else dctx
            rows = plan.rows if packed else B * S
            p, _, lse = attn_args(q, lengths, B, S, NH)
            ctx = torch.full((rows, H), 77.0, dtype=torch.bfloat16, device=DEV)
            dqkv = torch.full((rows, 3 * H), 77.0, dtype=torch.bfloat16, device=DEV)
            delta = torch.zeros((B, NH, S), dtype=torch.float32, device=DEV)
            colp = torch.full((B * QT * 4, 3 * H), 3.0, dtype=torch.float32, device=DEV)
            p.ctx = ctx.data_ptr()
            p.dctx, p.lddctx, p.delta, p.dqkv, p.lddqkv = d.data_ptr(), H, delta.data_ptr(), dqkv.data_ptr(), 3 * H
            p.colpart, p.colpart_accumulate = colp.data_ptr(), 0
            if packed:
                p.row_start = plan.row_start.data_ptr()
            assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 0
            assert L.plb_launch_attn_bwd(C.byref(p), stream()) == 0
            torch.cuda.synchronize()
            out[packed] = (ctx, dqkv, lse, colp)
        (c0, g0, l0, k0), (c1, g1, l1, k1) = out[False], out[True]
        assert torch.equal(c1[pr], c0[dr]) and torch.equal(g1[pr], g0[dr])
        valid = qmask.reshape(B, 1, S).expand(B, NH, S)
        assert torch.equal(l1[valid], l0[valid])
        # slot rows behind the length: finite context, exactly zero gradient (what the padded rows of the padded call hold)
        slot_tail = hole.clone()
        slot_tail[plan.used:] = False
        assert bool(torch.isfinite(c1[slot_tail].float()).all()) and float(g1[slot_tail].float().abs().max()) == 0.0
        # the tail behind the last slot belongs to no workgroup
        assert bool((c1[plan.used:] == 77.0).all()) and bool((g1[plan.used:] == 77.0).all())
        # bias-gradient partials: what the engine sums is the column sum of the valid rows in both layouts
        assert torch.allclose(k1.double().sum(0), g1[pr].double().sum(0), rtol=1e-5, atol=1e-3 * float(k0.abs().max()))
        assert torch.allclose(k1.double().sum(0), k0.double().sum(0), rtol=1e-5, atol=1e-3 * float(k0.abs().max()))
    finally:
        L.plb_set_attn_bwd_fused(-1)


def test_packed_attention_needs_lengths():
    L = _lib.lib()
    qkv = randbf(256, 3 * 64, seed=1)
    p, _, _ = attn_args(qkv, None, 2, 128, 1)
    p.row_start = torch.zeros(3, dtype=torch.int32, device=DEV).data_ptr()
    assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 1


def test_packed_embedding_kernels_are_bit_equal_to_the_padded_ones():
    """Forward rows, the scatter into the word / position tables (same lists, same order: pad positions only ever added
    exact zeros) bit for bit; rows without a token are zeros in the forward output and in dx."""
    L = _lib.lib()
    B, S, E, V, P, nblocks = len(LENS), 512, 128, 188, 512, 64
    plan = _plan(LENS, S)
    pr, dr, hole = _row_index(plan)
    lengths = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, V, (B, S), generator=g)
    ids[torch.rand(B, S, generator=g) < 0.3] = 3                 # a few ids own most of the tokens
    valid = torch.arange(S)[None, :] < torch.tensor(LENS)[:, None]
    ids[~valid] = 0                                              # the collater's zero pad
    ids = ids.to(DEV)
    tabs = {k: torch.randn(*shp, generator=g).to(DEV) for k, shp in
            dict(word=(V, E), pos=(P, E), type0=(E,), gamma=(E,), beta=(E,)).items()}
    dy = randbf(B * S, E, seed=9) * valid.reshape(-1, 1).to(DEV).to(torch.bfloat16)   # no loss behind the lengths
    res = {}
    for packed in (False, True):
        T = plan.rows if packed else B * S
        out = torch.full((T, E), 7.0, dtype=torch.bfloat16, device=DEV)
        dx = torch.full((T, E), 7.0, device=DEV)
        part = torch.zeros((nblocks, 2 * E), device=DEV)
        dword, dpos = torch.full((V, E), 7.0, device=DEV), torch.full((P, E), 7.0, device=DEV)
        d = _pack_rows(dy, plan, 5.0) if packed else dy
        p = _lib.PlbEmbed()
        p.ids, p.T, p.S, p.E, p.V = ids.data_ptr(), T, S, E, V
        p.word, p.pos, p.type0, p.gamma, p.beta = (tabs[k].data_ptr() for k in ("word", "pos", "type0", "gamma", "beta"))
        p.eps, p.out, p.ldo = 1e-12, out.data_ptr(), E
        p.dout, p.lddo, p.dx, p.dword, p.dpos = d.data_ptr(), E, dx.data_ptr(), dword.data_ptr(), dpos.data_ptr()
        p.partials, p.nblocks = part.data_ptr(), nblocks
        if packed:
            p.row_start, p.lengths, p.B = plan.row_start.data_ptr(), lengths.data_ptr(), B
        assert L.plb_launch_embed_fwd(C.byref(p), stream()) == 0
        assert L.plb_launch_embed_bwd(C.byref(p), stream()) == 0
        assert L.plb_launch_embed_scatter(C.byref(p), P, stream()) == 0
        torch.cuda.synchronize()
        res[packed] = (out, dx, part, dword, dpos)
    (o0, x0, p0, w0, s0), (o1, x1, p1, w1, s1) = res[False], res[True]
    assert torch.equal(o1[pr], o0[dr]) and torch.equal(x1[pr], x0[dr])
    assert float(o1[hole].float().abs().max()) == 0.0 and float(x1[hole].abs().max()) == 0.0   # the defined value: zeros
    assert torch.equal(w1, w0) and torch.equal(s1, s0)
    assert torch.allclose(p1.sum(0), p0.sum(0), rtol=1e-4, atol=1e-4 * float(p0.sum(0).abs().max()))


def test_packed_loss_rows_and_unpack_kernels():
    L = _lib.lib()
    B, S = len(LENS), 512
    plan = _plan(LENS, S)
    pr, dr, hole = _row_index(plan)
    lengths = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    rs = np.random.RandomState(0)
    idx = [sorted(rs.choice(n, size=max(1, n // 7), replace=False).tolist()) if b != 3 else [] for b, n in enumerate(LENS)]
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    n = int(off[-1])
    labels = torch.randint(1, 178, (B, S)).to(DEV)
    off_t, flat_t = torch.as_tensor(off).to(DEV), torch.as_tensor(flat).to(DEV)
    got = {}
    for packed in (False, True):
        rows, tgt = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
        w = torch.zeros(n, device=DEV)
        if packed:
            rc = L.plb_launch_ce_prepare_packed(off_t.data_ptr(), flat_t.data_ptr(), labels.data_ptr(), B, S,
                                                plan.row_start.data_ptr(), rows.data_ptr(), tgt.data_ptr(), w.data_ptr(), stream())
        else:
            rc = L.plb_launch_ce_prepare(off_t.data_ptr(), flat_t.data_ptr(), labels.data_ptr(), B, S, rows.data_ptr(),
                                         tgt.data_ptr(), w.data_ptr(), stream())
        assert rc == 0
        torch.cuda.synchronize()
        got[packed] = (rows.cpu().numpy(), tgt, w)
    want = np.concatenate([plan.row_start_host[b] + np.asarray(ix, np.int64) for b, ix in enumerate(idx)])
    assert np.array_equal(got[True][0], want)
    assert torch.equal(got[True][1], got[False][1]) and torch.equal(got[True][2], got[False][2])
    # unpack: bf16 and fp32 sources, padded stride, zeros at the pad positions
    for is_bf16 in (1, 0):
        Cc, ld = 178, 184
        src = torch.randn(plan.rows, ld, device=DEV)
        src = src.to(torch.bfloat16) if is_bf16 else src
        dst = torch.full((B, S, Cc), 9.0, device=DEV)
        assert L.plb_launch_unpack_rows(src.data_ptr(), is_bf16, ld, plan.row_start.data_ptr(), lengths.data_ptr(), B, S, Cc,
                                        dst.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        flat_dst = dst.reshape(B * S, Cc)
        assert torch.equal(flat_dst[dr], src[pr][:, :Cc].float())
        pad = torch.ones(B * S, dtype=torch.bool, device=DEV)
        pad[dr] = False
        assert float(flat_dst[pad].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------- engine level
def _step_inputs(g):
    idx = [list(map(int, x)) for x in g["index"]]
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    return g["masked"], g["labels"], np.asarray([int(x) for x in g["lengths"]], np.int32), off, flat, int(off[-1])


def _engine(g, **kw):
    ocfg, pcfg, sd = golden_cfg(g)
    B, S = g["labels"].shape
    eng = HipEngine(pcfg, int(g["num_phonemes"]), int(g["num_tokens"]), max_batch=kw.get("max_batch", B),
                    max_seq=kw.get("max_seq", S))
    eng.load_state_dict(sd)
    return eng


@pytest.mark.parametrize("prune", [1, 0])
@pytest.mark.parametrize("ln_fuse", ["both", "off"])
@pytest.mark.parametrize("name", ["real_s512_b32_ragged", "real_s512_b2_ragged"])
def test_packed_path_against_reference_probes(name, ln_fuse, prune, monkeypatch):
    """The reference-captured ragged fixtures through the packed path, with exactly the bounds of
    test_real_model_against_reference_probes: probe logits 3e-2, gradient norms 3e-2 relative, gradient probes 0.1 of the
    tensor maximum, loss trajectory rtol 1e-3, no LayerNorm hand-off time-outs; LayerNorm fused into the GEMMs and
    standalone, last application on the masked rows and on all rows. (32 samples: 12,288 rows instead of 16,384, the
    fused forms; 2 samples: 896 instead of 1,024, which only the 128-row granularity offers: standalone LayerNorm.)"""
    monkeypatch.setenv("PLBERT_LN_FUSE", ln_fuse)
    L = _lib.lib()
    g = load_golden(name)
    masked, labels, lens, off, flat, n = _step_inputs(g)
    plan = _plan(lens, masked.shape[1])
    steps = 2
    L.plb_set_prune_last(prune)
    try:
        eng = _engine(g)
        _, ph, _ = eng.forward(masked, lens, packing=plan)
        assert eng.last_call_rows() == (plan.rows, masked.size)
        ph = ph.cpu().numpy()
        assert np.abs(ph[g["probe_b"], g["probe_s"]] - g["probe_logits"]).max() < 3e-2
        losses = []
        for step in range(1, steps + 1):
            loss = eng.loss_fwd_bwd(masked, labels, lens, off, flat, n, packing=plan)
            if step == 1:
                torch.cuda.synchronize()
                assert eng.last_call_rows() == (plan.rows, masked.size) and plan.rows < masked.size
                rows, of = eng.last_application_rows()
                assert of == plan.rows and ((rows < of) if prune else (rows == of))
                for k, ref in zip(g["grad_names"], g["grad_l2"]):
                    if str(k) == KEY_BIAS:
                        continue  # exactly-zero gradient (softmax is invariant to a per-query shift of the scores)
                    got = float(eng.view(str(k), of=eng.grads).double().norm())
                    assert abs(got - ref) <= 3e-2 * ref + 1e-6, (k, got, ref)
                    flatg = eng.view(str(k), of=eng.grads).flatten().cpu().numpy()
                    pv = g["gprobe_val/" + str(k)]
                    assert np.abs(flatg[g["gprobe_idx/" + str(k)]] - pv).max() <= 0.1 * np.abs(flatg).max() + 1e-7, k
            losses.append(float(loss.item()))
            eng.adamw_step(step, lr=7e-5)
        assert np.allclose(losses, g["losses"][:steps], rtol=1e-3), (losses, g["losses"][:steps])
        assert eng.status()["ln_exchange_timeouts"] == 0
    finally:
        L.plb_set_prune_last(-1)


@pytest.mark.parametrize("name", ["real_s512_b32_ragged", "real_s512_b2_ragged"])
def test_packed_equals_padded_as_two_bf16_evaluations(name):
    """Same engine weights, packed against padded: each valid row's arithmetic is unchanged, the weight-gradient sums run
    over other row counts and splits — the bar test_last_application_on_masked_rows_only_equals_the_full_evaluation sets
    for two bf16 evaluations of one function: loss 1e-4 relative, every trainable tensor 1.5e-2 relative L2; the loss-only
    call gives the packed training call's loss bit for bit."""
    g = load_golden(name)
    masked, labels, lens, off, flat, n = _step_inputs(g)
    plan = _plan(lens, masked.shape[1])
    eng = _engine(g)
    l_pad = float(eng.loss_fwd_bwd(masked, labels, lens, off, flat, n).item())
    assert eng.last_call_rows() == (masked.size, masked.size)
    g_pad = eng.grads[: eng.trainable].clone()
    l_val = float(eng.loss_fwd(masked, labels, lens, off, flat, n, packing=plan).item())
    assert eng.last_call_rows() == (plan.rows, masked.size)
    l_pk = float(eng.loss_fwd_bwd(masked, labels, lens, off, flat, n, packing=plan).item())
    g_pk = eng.grads[: eng.trainable].clone()
    assert l_val == l_pk
    assert abs(l_pk - l_pad) <= 1e-4 * l_pad, (l_pk, l_pad)
    for k, (o, sz, shp) in eng.layout.items():
        if o + sz > eng.trainable or k == KEY_BIAS:
            continue
        assert rel_l2(g_pk[o:o + sz], g_pad[o:o + sz]) < 1.5e-2, (k, rel_l2(g_pk[o:o + sz], g_pad[o:o + sz]))
    assert eng.status()["ln_exchange_timeouts"] == 0


def _oracle_case(B, S, lengths, seed, empty=()):
    rs = np.random.RandomState(seed)
    labels, masked, idx = np.zeros((B, S), np.int64), np.zeros((B, S), np.int64), []
    for b, n in enumerate(lengths):
        labels[b, :n] = rs.randint(1, 185, size=n)
        masked[b, :n] = labels[b, :n]
        ii = sorted(rs.choice(n, size=max(1, n // 6), replace=False).tolist()) if b not in empty else []
        masked[b, ii] = 185
        idx.append(ii)
    return labels, masked, idx


# The first five are the shapes of test_edge_shapes_against_oracle and test_against_oracle_random_shapes. None of them can
# pack (sequences shorter than one 128-row slot, one full sample): given a plan they must run PADDED, which is all they
# check here — at this file's small config, not at those tests' own. The packed path is exercised by the last three: ragged
# shapes that do pack — a single token beside long samples, lengths around the 64-key and 128-row tiles, S no multiple of
# 64, an empty index list.
ORACLE_SHAPES = [(1, 1, [1]), (1, 512, [512]), (5, 33, [33, 32, 2, 1, 1]), (3, 65, [65, 64, 63]), (5, 90, [90, 77, 64, 13, 1]),
                 (5, 300, [300, 129, 128, 65, 1]), (4, 512, [512, 257, 63, 2]), (6, 200, [200, 127, 64, 13, 1, 1])]


@pytest.mark.parametrize("B,S,lengths", ORACLE_SHAPES)
def test_packed_shapes_against_oracle(B, S, lengths):
    """Bounds of test_edge_shapes_against_oracle: logits 3e-2 on valid positions, loss 1e-3, gradients 5e-2 of the tensor's
    norm + 1e-4 of the step's largest."""
    ocfg = onp.Config(embedding_size=64, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2)
    pcfg = plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)
    sd = plbert_amd.deterministic_state_dict(pcfg, 188, seed=13)
    labels, masked, idx = _oracle_case(B, S, lengths, 100 * B + S, empty=(3,) if B > 4 else ())
    loss_ref, pred_ref, G = onp.loss_and_grads(ocfg, sd, masked, labels, lengths, idx)
    plan = packing_plan(lengths, S)
    assert plan.packed == (S >= 200 and B > 1)
    eng = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S)
    eng.load_state_dict(sd)
    lens = np.asarray(lengths, np.int32)
    _, ph, _ = eng.forward(masked, lens, packing=plan)
    assert eng.last_call_rows() == ((plan.rows if plan.packed else B * S), B * S)
    v = np.arange(S)[None, :] < lens[:, None]
    ph = ph.cpu().numpy()
    assert np.abs(ph[v] - pred_ref[v]).max() < 3e-2
    if plan.packed:
        assert np.abs(ph[~v]).max() == 0.0
    off, flat = plbert_amd.masked_indices_to_csr(idx)
    loss = eng.loss_fwd_bwd(masked, labels, lens, off, flat, int(off[-1]), packing=plan)
    assert abs(float(loss.item()) - float(loss_ref)) / float(loss_ref) < 1e-3
    scale = max(float(np.sqrt((np.asarray(w, np.float64) ** 2).sum())) for w in G.values())
    for k, want in G.items():
        got = eng.view(k, of=eng.grads).cpu().double()
        want = torch.as_tensor(want).double()
        err = float((got - want).norm())
        assert err <= 5e-2 * float(want.norm()) + 1e-4 * scale, (k, err, float(want.norm()), scale)


def test_packed_call_without_masked_positions_gives_zero_loss_and_gradients():
    g = load_golden("real_s512_b2_ragged")
    masked, labels, lens, off, flat, n = _step_inputs(g)
    eng = _engine(g)
    eng.grads.fill_(1.0)
    loss = eng.loss_fwd_bwd(masked, labels, lens, np.zeros_like(off), flat[:0], 0, packing=_plan(lens, 512))
    assert float(loss.item()) == 0.0 and float(eng.grads[: eng.trainable].abs().max()) == 0.0


def test_packed_call_after_a_larger_call_equals_a_fresh_engine():
    """Rows of the packed axis that hold no token (slot ends, the tail up to the call's row count) are written by no
    attention workgroup, and the workspace keeps what a larger call left there; the token-major weight-gradient GEMMs
    read every row. Gradients after a full 32 x 512 call must equal those of a fresh engine bit for bit."""
    g = load_golden("real_s512_b32_ragged")
    masked, labels, lens, off, flat, n = _step_inputs(g)
    plan = _plan(lens, 512)
    fresh = _engine(g)
    l0 = float(fresh.loss_fwd_bwd(masked, labels, lens, off, flat, n, packing=plan).item())
    g0 = fresh.grads[: fresh.trainable].clone()
    used = _engine(g)
    big_labels, big_masked, _, big_idx = plbert_amd.synthetic_batch(32, 512, seed=77)
    boff, bflat = plbert_amd.masked_indices_to_csr(big_idx)
    used.loss_fwd_bwd(big_masked, big_labels, None, boff, bflat, int(boff[-1]))
    assert used.last_call_rows() == (32 * 512, 32 * 512)
    l1 = float(used.loss_fwd_bwd(masked, labels, lens, off, flat, n, packing=plan).item())
    assert l1 == l0 and torch.equal(used.grads[: used.trainable], g0)


def test_packed_forward_outputs():
    """Valid positions equal the padded outputs bit for bit (stronger than the forward tests' 3e-2: every forward launch is
    row-independent — GEMM rows, LayerNorm rows, attention on the same tiles — and both calls take the fused forms), pad
    positions exactly zero, pooler output equal (it reads hidden[b, 0, :], a valid position of every sample)."""
    g = load_golden("real_s512_b32_ragged")
    masked, labels, lens, off, flat, n = _step_inputs(g)
    plan = _plan(lens, 512)
    eng = _engine(g)
    h0, p0, _ = eng.forward(masked, lens, want_hidden=True)
    h1, p1, _ = eng.forward(masked, lens, want_hidden=True, packing=plan)
    v = torch.as_tensor(np.arange(512)[None, :] < lens[:, None]).to(DEV)
    assert eng.last_call_rows() == (plan.rows, masked.size)
    print("max |packed - padded| on valid positions: logits", float((p1[v] - p0[v]).abs().max()), "hidden",
          float((h1[v] - h0[v]).abs().max()))
    assert torch.equal(p1[v], p0[v]) and torch.equal(h1[v], h0[v])
    assert float(p1[~v].abs().max()) == 0.0 and float(h1[~v].abs().max()) == 0.0
    assert torch.equal(eng.pooler(h1), eng.pooler(h0))


def test_packed_step_is_graph_capturable():
    """As test_step_is_graph_capturable: for a fixed plan the packed call has no host synchronisation or allocation."""
    g = load_golden("real_s512_b2_ragged")
    eng = _engine(g)
    masked, labels, lens, off, flat, n = _step_inputs(g)
    plan = _plan(lens, 512)
    dev = eng.device
    args = [torch.as_tensor(masked).to(dev), torch.as_tensor(labels).to(dev), torch.as_tensor(lens).to(dev),
            torch.as_tensor(off).to(dev), torch.as_tensor(flat).to(dev), n]
    eng.loss_fwd_bwd(*args, packing=plan)
    torch.cuda.synchronize()
    loss_eager = float(eng._loss.item())
    grads_eager = eng.grads[: eng.trainable].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.loss_fwd_bwd(*args, packing=plan)
    eng.grads.zero_()
    eng._loss.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert eng.last_call_rows() == (plan.rows, masked.size)
    assert float(eng._loss.item()) == loss_eager
    assert torch.equal(eng.grads[: eng.trainable], grads_eager)


def test_calls_that_run_padded_although_given_a_plan():
    """A full-length batch and an fp8 call (a plan of 896 rows that would pack) report rows == B*S and equal the call without
    a plan bit for bit. Dual-head calls: the next test."""
    # full-length batch
    g = load_golden("real_s128_b8")
    masked, labels, lens, off, flat, n = _step_inputs(g)
    B, S = masked.shape
    full = np.full(B, S, np.int32)
    plan = packing_plan(full, S)
    assert not plan.packed
    eng = _engine(g)
    l0 = float(eng.loss_fwd_bwd(masked, labels, full, off, flat, n).item())
    g0 = eng.grads[: eng.trainable].clone()
    l1 = float(eng.loss_fwd_bwd(masked, labels, full, off, flat, n, packing=plan).item())
    assert eng.last_call_rows() == (B * S, B * S) and l1 == l0 and torch.equal(eng.grads[: eng.trainable], g0)
    # fp8 mode, ragged batch: calibration call and fp8 call
    g = load_golden("real_s512_b2_ragged")
    masked, labels, lens, off, flat, n = _step_inputs(g)
    plan = _plan(lens, 512)
    res = []
    for pk in (None, plan):
        eng = _engine(g)
        eng.set_fp8(True)
        ls = [float(eng.loss_fwd_bwd(masked, labels, lens, off, flat, n, packing=pk).item()) for _ in range(3)]
        assert eng.last_call_rows() == (masked.size, masked.size)
        res.append((ls, eng.grads[: eng.trainable].clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])


def test_dual_head_calls_run_padded_although_their_plan_packs():
    """A dual-head engine (token head of 300 classes on the 2 x 512 ragged fixture's model) and a plan that really packs
    (896 of 1,024 rows): the token loss reads every position with padded-layout weights, so calls with token targets /
    token logits must run padded — rows == B*S, results those of the call without a plan bit for bit. Both calls below
    hand the plan to the library (plb_loss_fwd_packed with token_ids, plb_forward_packed with token_logits); the dual-head
    TRAINING call has no packed entry point. The same engine does pack its phoneme-only calls."""
    g = load_golden("real_s512_b2_ragged")
    _, pcfg, _ = golden_cfg(g)
    masked, labels, lens, off, flat, n = _step_inputs(g)
    B, S = masked.shape
    NT = 300
    plan = _plan(lens, S)
    assert plan.packed and plan.rows == 896 < B * S
    eng = HipEngine(pcfg, int(g["num_phonemes"]), NT, max_batch=B, max_seq=S)
    eng.load_state_dict(plbert_amd.reference_init_state_dict(pcfg, int(g["num_phonemes"]), NT, seed=0))
    tok = np.random.RandomState(1).randint(0, NT, size=(B, S))
    out = []
    for pk in (None, plan):
        loss = float(eng.loss_fwd(masked, labels, lens, off, flat, n, token_ids=tok, packing=pk).item())
        assert eng.last_call_rows() == (B * S, B * S)
        parts = eng.loss_parts.clone()
        _, ph, tk = eng.forward(masked, lens, want_token=True, packing=pk)
        assert eng.last_call_rows() == (B * S, B * S)
        l_tr = float(eng.loss_fwd_bwd(masked, labels, lens, off, flat, n, token_ids=tok, packing=pk).item())
        assert eng.last_call_rows() == (B * S, B * S)
        out.append((loss, parts, ph, tk, l_tr, eng.grads.clone()))
    a, b = out
    assert a[0] == b[0] and a[4] == b[4] and a[0] == a[4] and float(a[1][1]) > 0        # (a token term was computed)
    assert all(torch.equal(x, y) for x, y in zip(a[1:4] + a[5:], b[1:4] + b[5:]))
    eng.loss_fwd(masked, labels, lens, off, flat, n, packing=plan)                       # phoneme-only: packs
    assert eng.last_call_rows() == (plan.rows, B * S)


def test_feeder_attaches_the_plan_and_the_run_trains_packed():
    """The input pipeline with packing on (what run.train uses): every ragged batch arrives with the plan of its own
    lengths — made where the batch is staged, its row table in the feeder's per-slot buffers — and a trainer fed by it
    follows the padded trainer's losses."""
    from plbert_amd import data as pdata
    from plbert_amd.pipeline import DeviceFeeder
    from plbert_amd.train import PLBertTrainer
    g = load_golden("masking")
    docs = [{"phonemes": d.split("\x1f")} for d in g["docs"] if len(d) > 0] * 6

    def loader():
        torch.manual_seed(3)
        pdata.seed_reference_streams(1)
        return plbert_amd.build_dataloader(docs, batch_size=4, device="cpu", use_token_ids=False, num_workers=0, decisions=False,
                                           dataset_config=dict(max_seq_length=256, word_separator=87, word_pred_prob=0.15,
                                                               phoneme_mask_prob=0.8, replace_prob=0.1))[0]
    cfg = plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                  intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)
    losses = {}
    for packed in (False, True):
        tr = PLBertTrainer(cfg, 188, max_batch=4, max_seq=256, lr=1e-3, seed=1, packed=packed)
        ls, k = [], 0
        for b in DeviceFeeder(loader(), vocab_size=188, packed=packed):
            if packed:
                want = packing_plan(b.lengths_host, b.masked.shape[1])
                assert want.packed and b.packing is not None and b.packing.rows == want.rows
                assert np.array_equal(b.packing.row_start.cpu().numpy(), want.row_start_host)
            else:
                assert b.packing is None
            ls.append(float(tr.step(b).item()))
            rows, of = tr.engine.last_call_rows()
            assert (rows < of) == packed and of == b.masked.numel()
            k += 1
        assert k > 4
        losses[packed] = ls
    assert np.allclose(losses[True], losses[False], rtol=2e-3), (losses[True], losses[False])


def test_trainer_packed_switch():
    """PLBertTrainer(packed=True): stage_batch adds the plan, the step runs packed and trains like the padded trainer."""
    from plbert_amd.train import PLBertTrainer
    g = load_golden("real_s512_b2_ragged")
    ocfg, pcfg, sd = golden_cfg(g)
    idx = [list(map(int, x)) for x in g["index"]]
    lengths = [int(x) for x in g["lengths"]]
    losses = {}
    for packed in (False, True):
        tr = PLBertTrainer(pcfg, int(g["num_phonemes"]), max_batch=2, max_seq=512, lr=7e-5, device=DEV, state_dict=sd,
                           packed=packed)
        batch = tr.stage_batch(g["labels"], g["masked"], lengths, idx)
        assert (batch.packing is not None) == packed
        losses[packed] = [float(tr.step(batch).item()) for _ in range(2)]
        rows, of = tr.engine.last_call_rows()
        assert (rows < of) == packed
        assert float(tr.loss_only(batch).item()) > 0
    assert np.allclose(losses[True], losses[False], rtol=1e-3) and np.allclose(losses[True], g["losses"][:2], rtol=1e-3)
