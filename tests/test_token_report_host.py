"""Token report, the parts that need no GPU: the instrument (tests/token_report_ref.py) against torch and against hand-written
tie cases; the workspace plb_token_report adds (proportional to the row capacity, independent of the vocabulary, none without
a token head — plb_create is host-only); the ctypes mirror of PlbTokenReport against the header."""
import ctypes as C

import numpy as np
import pytest
import torch

import c_header
import token_report_ref as ref
from plbert_amd import _lib


def test_instrument_against_torch_on_rows_without_ties():
    g = np.random.default_rng(5)
    n, NT = 37, 301
    z = g.normal(0, 3, size=(n, NT))
    assert all(len(np.unique(r)) == NT for r in z)
    tgt = g.integers(0, NT, size=n)
    tgt[0] = int(z[0].argmax())
    zt = torch.from_numpy(z)
    lsm = torch.log_softmax(zt, -1)
    for k in (0, 1, 5, 8):
        got = ref.report(z, tgt, k)
        v, i = torch.topk(zt, k, dim=-1) if k else (zt[:, :0], torch.zeros((n, 0), dtype=torch.int64))
        assert np.array_equal(got.topk_ids, i.numpy().astype(np.int32))
        assert np.allclose(got.topk_logprob, torch.gather(lsm, 1, i).numpy(), rtol=0, atol=1e-12)
        assert np.allclose(got.lse, torch.logsumexp(zt, -1).numpy(), rtol=0, atol=1e-12)
        assert np.allclose(got.target_logprob, lsm[torch.arange(n), torch.from_numpy(tgt)].numpy(), rtol=0, atol=1e-12)
        rank = (z > z[np.arange(n), tgt][:, None]).sum(1)
        assert np.array_equal(got.target_pos, np.where(rank < k, rank, -1))
        assert got.totals.tolist() == [n, int(((rank == 0) & (k > 0)).sum()), int((rank < k).sum())]


def test_instrument_on_hand_written_cases():
    z = np.array([[1.0, 3.0, 3.0, 0.0, 3.0],          # ties: the lowest index first
                  [2.0, 2.0, 2.0, 2.0, 2.0],          # all equal: 0, 1, 2, ...
                  [0.0, np.nan, 5.0, 1.0, 1.0],       # a NaN row
                  [9.0, 8.0, 7.0, 6.0, 5.0],          # a position without a row (values ignored)
                  [0.0, 1.0, 2.0, 3.0, 4.0]])
    tgt = np.array([4, 3, 2, 0, 7])                   # the last target lies outside the vocabulary
    rows = np.array([10, 0, 3, -1, 3])
    r = ref.report(z, tgt, 3, rows)
    assert r.topk_ids.tolist() == [[1, 2, 4], [0, 1, 2], [-1, -1, -1], [-1, -1, -1], [4, 3, 2]]
    assert r.target_pos.tolist() == [2, -1, -1, -1, -1]
    assert r.totals.tolist() == [4, 0, 1]
    assert np.isnan(r.topk_logprob[2]).all() and np.isneginf(r.topk_logprob[3]).all()
    assert np.isnan(r.lse[[2, 3]]).all() and np.isnan(r.target_logprob[[2, 3, 4]]).all()
    assert np.isclose(r.lse[1], 2.0 + np.log(5.0)) and np.isclose(r.target_logprob[1], -np.log(5.0))
    # a list longer than the vocabulary: -1 / -inf behind it
    r8 = ref.report(z[:2], tgt[:2], 8)
    assert r8.topk_ids[0].tolist() == [1, 2, 4, 0, 3, -1, -1, -1] and np.isneginf(r8.topk_logprob[0, 5:]).all()
    assert r8.target_pos.tolist() == [2, 3]
    # target_pos == 0 is EXACT top-1: a target that ties the maximum at a higher index does not count
    assert ref.report(z[:1], [2], 5).totals.tolist() == [1, 0, 1] and ref.report(z[:1], [1], 5).totals.tolist() == [1, 1, 1]
    # no targets: no target outputs, no hits
    r0 = ref.report(z, None, 2, rows)
    assert (r0.target_pos == -1).all() and np.isnan(r0.target_logprob).all() and r0.totals.tolist() == [4, 0, 0]


def test_instrument_prepare_and_strips():
    offsets, flat = np.array([0, 2, 2, 5]), np.array([0, 3, 1, 2, 6])
    lengths, tok = np.array([4, 7, 6]), np.arange(21).reshape(3, 7)
    rows, tgt = ref.prepare(offsets, flat, lengths, None, tok, 5, 3, 7)
    assert rows.tolist() == [0, 3, 15, 16, -1] and tgt.tolist() == [0, 3, 15, 16, -1]
    rows, tgt = ref.prepare(offsets, flat, lengths, np.array([0, 128, 256, 384]), None, 5, 3, 7)
    assert rows.tolist() == [0, 3, 257, 258, -1] and (tgt == -1).all()
    rows, _ = ref.prepare(None, None, lengths, None, None, 21, 3, 7)
    assert rows.tolist() == [0, 1, 2, 3, -1, -1, -1] + list(range(7, 14)) + [14, 15, 16, 17, 18, 19, -1]
    assert ref.strips(16384, 64000) == 4 and ref.strips(1, 64000) == 16 and ref.strips(300, 129) == 2
    assert ref.strips(128, 5000, 3) == 3 and ref.strips(128, 5 * 128, 4) == 3 and ref.strips(128, 5, 16) == 1


def _ws(num_tokens, max_batch, max_seq, infer):
    L = _lib.lib()
    c = _lib.PlbConfig(188, 128, 768, 12, 2048, 2, 512, 2, 1e-12, 188, num_tokens, max_batch, max_seq, 1 if infer else 0)
    h = C.c_void_p()
    assert L.plb_create(C.byref(c), C.byref(h)) == 0, L.plb_last_error()
    ws = int(L.plb_workspace_bytes(h))
    L.plb_destroy(h)
    return ws


def test_the_library_and_the_instrument_agree_on_the_strip_policy():
    L = _lib.lib()
    for n in (1, 127, 129, 300, 4096, 16384):
        for NT in (5, 96, 128, 129, 1000, 5000, 64000):
            for forced in (0, 1, 3, 16):
                assert L.plb_token_topk_strips(n, NT, forced) == ref.strips(n, NT, forced), (n, NT, forced)
    assert L.plb_token_topk_strips(0, 5, 0) == 0 and int(L.plb_token_topk_scratch_bytes(128)) <= 128 * 1300 + 256


@pytest.mark.parametrize("infer", [False, True])
def test_workspace_growth_with_the_row_capacity(infer):
    """What the report adds is proportional to Tcap and stays within 2 KiB per row; an engine without a token head gets
    none of it. Measured as a difference of differences: everything else that grows with the rows grows alike in an engine
    whose token head is one 256-column tile wide and in one with none, except the token head's own per-row regions, which the
    test restates (engine.cpp: o_tlrows, o_tpmax, o_tpsum, o_ttl, o_tlse, o_tw, o_ttgt; training: o_tdl, o_tcolp)."""
    NT, S = 256, 512
    small, big = 4, 8                                                  # Tcap 2048 -> 4096
    dT = (big - small) * S
    per_row_head = 4 + 4 + 4 + 4 + 4 + 4 + 8 + (0 if infer else 2 * NT + 2 * NT * 4 // 128)
    grow_tok = _ws(NT, big, S, infer) - _ws(NT, small, S, infer)
    grow_none = _ws(0, big, S, infer) - _ws(0, small, S, infer)
    extra = grow_tok - grow_none - per_row_head * dT - (dT // 4) * 2 * 4   # (o_rep_tok: plb_masked_report's, per 4 rows)
    if not infer:
        # training engines also size the weight-gradient slab by the widest shape; at these sizes the token head's is not it
        assert _ws(NT, small, S, False) - _ws(0, small, S, False) < 64 << 20
    assert 0 < extra <= 2048 * dT, (extra, extra / dT)
    assert abs(extra / dT - 1291) < 2, extra / dT                      # 16 x (64 + 16) + 3 + 4 + 4, and 256-B rounding


def test_workspace_growth_with_the_vocabulary_is_the_old_regions_alone():
    """num_tokens 1000 -> 64000 at a fixed row capacity, inference-only engine: the growth is that of the regions that were
    there before — the flat bf16 weight copy, the padded bias and the per-tile row statistics of the fused head."""
    B, S, H = 4, 512, 768
    Tp = B * S
    got = _ws(64000, B, S, True) - _ws(1000, B, S, True)

    def r256(x):
        return (x + 255) // 256 * 256

    def old(nt):
        ntp = r256(nt)
        return (nt * H + nt) * 2, ntp * 4, Tp * (ntp // 256) * 4
    w1, b1, p1 = old(64000)
    w0, b0, p0 = old(1000)
    want = (w1 - w0) + (r256(b1) - r256(b0)) + 2 * (r256(p1) - r256(p0))
    assert abs(got - want) <= 256, (got, want)                          # (the flat copy's own rounding to 256 B)


def test_struct_mirror_against_the_header():
    hdr = c_header.public()
    fields = hdr.structs["PlbTokenReport"]
    assert [f.name for f in fields] == [n for n, _ in _lib.PlbTokenReport._fields_]
    assert all(f.depth == 1 for f in fields) and all(t is C.c_void_p for _, t in _lib.PlbTokenReport._fields_)
    assert C.sizeof(_lib.PlbTokenReport) == 7 * C.sizeof(C.c_void_p)
    assert [f.base for f in fields] == ["int32_t", "float", "float", "float", "int32_t", "float", "int32_t"]
    proto = hdr.protos["plb_token_report"]
    assert not c_header.signature_mismatch(hdr, proto, *_lib.PUBLIC["plb_token_report"],
                                           {"PlbPacking": _lib.PlbPacking, "PlbTokenReport": _lib.PlbTokenReport})
