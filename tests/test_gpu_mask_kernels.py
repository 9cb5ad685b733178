"""The masking kernels bit for bit (-m gpu): plb_launch_mask and plb_launch_apply_mask called directly with the PlbMask /
PlbApplyMask mirrors and compared, exactly, with the numpy restatements of tests/mask_ref.py (held on the CPU to the
published Philox4x32-10 vectors and to the masking distribution by tests/test_mask_ref_host.py).

mask_words_kernel is a pure function of (labels, lengths, seed, step, probabilities): both key halves, a full 32-bit step,
every wave boundary of its 512-thread workgroup, empty / one-phoneme pools and the probability edges are compared over the
whole [B,S]. apply_mask_kernel runs at its limits: S up to 1024 (four 256-position chunks of its compaction), crops that
cut words at both ends of the window or remove a sample, all and none of the positions modified. mask_compact_kernel runs
at B = 1 and B = 1024 behind both. Every output buffer is pre-filled with a sentinel and has sentinel pads on both sides."""
import ctypes as C

import numpy as np
import pytest
import torch

import mask_ref as mr
from gpu_util import stream
from plbert_amd import _lib

pytestmark = pytest.mark.gpu

PAD, SENT = 16, -7
PAIRS = ((1234, 7), (2 ** 40 + 99, 0), (3, 2 ** 32 - 1), (0xDEADBEEFCAFEF00D, 123456))
PROBS = (mr.DEFAULT_PROBS, (1.0, 0.5, 0.5), (1.0, 0.0, 1.0), (0.0, 0.8, 0.1))


class Out:
    """n elements a kernel may write, pre-filled with SENT, between two pads of SENT it may not."""

    def __init__(self, n, dtype):
        self.n = n
        self.buf = torch.full((PAD + n + PAD,), SENT, dtype=dtype, device="cuda")
        self.ptr = self.buf.data_ptr() + PAD * self.buf.element_size()

    def get(self, shape=None):
        a = self.buf[PAD:PAD + self.n].cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def pads_ok(self):
        return bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[PAD + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def _dev(a, dtype):
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(-1))
    return torch.from_numpy(a if a.size else np.zeros(1, dtype)).cuda()     # (an empty array still gets a valid pointer)


def _check_csr(what, B, S, lists, counts, idx, offsets, flat):
    want_counts, want_off, want_flat = mr.csr(lists)
    n = int(want_off[-1])
    assert np.array_equal(counts.get(), want_counts), f"{what}: counts"
    assert np.array_equal(offsets.get()[:B + 1], want_off), f"{what}: offsets"
    assert (offsets.get()[B + 1:] == SENT).all(), f"{what}: offsets past B + 1 were written"
    got = flat.get()
    assert np.array_equal(got[:n], want_flat), f"{what}: flat"
    assert (got[n:] == SENT).all(), f"{what}: flat past its {n} entries was written"
    pad = idx.get((B, S))
    for b in range(B):
        k = len(lists[b])
        assert np.array_equal(pad[b, :k], lists[b]) and (pad[b, k:] == SENT).all(), f"{what}: idx_padded row {b}"
    for o in (counts, idx, offsets, flat):
        assert o.pads_ok(), f"{what}: a pad was written"


# ---- plb_launch_mask ------------------------------------------------------------------------------------------------------
def _mask_args(lab, lengths, seed, step, probs, B=None, S=None):
    lab = np.asarray(lab, dtype=np.int64)
    B0, S0 = lab.shape
    B, S = B0 if B is None else B, S0 if S is None else S
    keep = dict(labels=_dev(lab, np.int64), lengths=_dev(lengths, np.int32) if lengths is not None else None,
                masked=Out(B0 * S0, torch.int64), counts=Out(B0, torch.int32), idx=Out(B0 * S0, torch.int32),
                offsets=Out(B0 + 3, torch.int32), flat=Out(B0 * S0, torch.int32))
    p = _lib.PlbMask()
    p.labels, p.lengths = keep["labels"].data_ptr(), keep["lengths"].data_ptr() if lengths is not None else None
    p.B, p.S, p.seed, p.step = B, S, seed, step
    p.word_pred_prob, p.mask_prob, p.replace_prob = probs
    p.mask_id, p.sep_id = mr.MASK_ID, mr.SEP_ID
    p.masked, p.counts, p.idx_padded, p.offsets, p.flat = (keep[k].ptr for k in ("masked", "counts", "idx", "offsets", "flat"))
    return p, keep


def _run_mask(what, lab, lengths, seed, step, probs=mr.DEFAULT_PROBS):
    B, S = lab.shape
    p, k = _mask_args(lab, lengths, seed, step, probs)
    rc = _lib.lib().plb_launch_mask(C.byref(p), stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    want, lists = mr.mask_words(lab, lengths, seed, step, probs)
    got = k["masked"].get((B, S))
    if not np.array_equal(got, want):
        b, i = (int(x) for x in np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: masked[{b}, {i}] is {int(got[b, i])}, the restatement has {int(want[b, i])} (label "
                             f"{int(lab[b, i])}); {int((got != want).sum())} positions differ")
    assert k["masked"].pads_ok()
    _check_csr(what, B, S, lists, k["counts"], k["idx"], k["offsets"], k["flat"])
    return want, lists


@pytest.mark.parametrize("S", [1, 63, 64, 65, 100, 512])
def test_mask_words_equals_the_restatement(S):
    changed = 0
    for B in (1, 3):
        lab, lengths = mr.random_labels(B, S, 100 + S + B)
        lengths[0] = S if S < 63 else S - 1 - (S % 7)                # the first row ends inside the last wave
        for seed, step in PAIRS:
            for given in (None, lengths):
                _, lists = _run_mask(f"S={S} B={B} seed={seed:#x} step={step} lengths={'given' if given else 'NULL'}",
                                     lab, given, seed, step)
                changed += sum(len(x) for x in lists)
    assert changed > 0 or S == 1


def test_mask_words_on_1024_samples():
    lab, lengths = mr.random_labels(1024, 64, 11)
    for seed, step in PAIRS[1:3]:
        _, lists = _run_mask(f"B=1024 seed={seed:#x}", lab, lengths, seed, step)
        assert sum(1 for x in lists if len(x)) > 300                 # the scan over 1024 counts has work to do
    _run_mask("B=1024 lengths=NULL", lab, None, *PAIRS[3])


def _hand_batch():
    """S = 512, one row per edge. Returns (labels, lengths)."""
    S = 512
    rs = np.random.RandomState(77)
    ph = lambda n: rs.randint(1, 185, size=n)   # noqa: E731
    rows, lengths = [], []

    def add(row, n):
        rows.append(np.asarray(row, dtype=np.int64))
        lengths.append(n)

    add(ph(S), S)                                                    # no separator: one 512-phoneme word across all 8 waves
    add(np.full(S, mr.SEP_ID), S)                                    # only separators: an empty pool
    r = mr.random_labels(1, S, 3)[0][0]
    r[0] = mr.SEP_ID
    add(r, S)                                                        # a separator at position 0
    r = ph(S)
    for a, b in ((5, 9), (62, 66), (200, 201), (255, 258), (300, 340), (509, 512)):
        r[a:b] = mr.SEP_ID
    add(r, S)                                                        # runs of consecutive separators, over wave edges too
    r = ph(S)
    r[[60, 70, 440, 455]] = mr.SEP_ID
    r[100:400:9] = mr.SEP_ID
    add(r, S)                                                        # words that straddle 63/64 and 447/448
    r = mr.random_labels(1, S, 4)[0][0]
    add(r, 0)                                                        # length 0
    add(r.copy(), 1)                                                 # length 1
    add(r.copy(), 511)                                               # length 511
    r = np.full(S, mr.SEP_ID)
    r[2] = 42
    r[5:] = ph(S - 5)
    add(r, 5)                                                        # a pool of one phoneme
    r = mr.random_labels(1, S, 6)[0][0]
    r[300:] = rs.randint(150, 188, size=S - 300)                     # garbage behind the length, mask and separator ids too
    add(r, 300)
    return np.stack(rows), lengths


@pytest.mark.parametrize("probs", PROBS)
def test_mask_words_hand_built_rows_and_probability_edges(probs):
    lab, lengths = _hand_batch()
    B, S = lab.shape
    for seed, step in PAIRS:
        want, lists = _run_mask(f"hand rows probs={probs} seed={seed:#x}", lab, lengths, seed, step, probs)
        phon = [np.flatnonzero(lab[b, :lengths[b]] != mr.SEP_ID) for b in range(B)]
        if probs == (1.0, 0.5, 0.5):
            assert all(np.array_equal(lists[b], phon[b]) for b in range(B))          # the index list is every phoneme
        elif probs == (1.0, 0.0, 1.0):
            assert all(np.array_equal(lists[b], phon[b]) for b in range(B)) and not (want[lab != mr.MASK_ID] == mr.MASK_ID).any()
            assert (want[8, 2] == 42)                                                 # the pool of one: replaced by itself
        elif probs == (0.0, 0.8, 0.1):
            assert np.array_equal(want, lab) and all(len(x) == 0 for x in lists)
        assert np.array_equal(want[9, 300:], lab[9, 300:]) and len(lists[5]) == 0
    if probs == mr.DEFAULT_PROBS:
        _run_mask("hand rows lengths=NULL", lab, None, *PAIRS[3], probs)


@pytest.mark.parametrize("B,S", [(1, 0), (1, 513), (0, 64), (1025, 64)])
def test_mask_refusals_write_nothing(B, S):
    lab, lengths = mr.random_labels(2, 64, 1)
    p, k = _mask_args(lab, lengths, 1, 1, mr.DEFAULT_PROBS, B=B, S=S)
    assert _lib.lib().plb_launch_mask(C.byref(p), stream()) != 0
    torch.cuda.synchronize()
    assert all(k[n].untouched() for n in ("masked", "counts", "idx", "offsets", "flat"))


# ---- plb_launch_apply_mask --------------------------------------------------------------------------------------------------
KINDS = ("crop", "all", "none", "gone", "short")


def _sample(kind, S, rs, with_tok):
    """One decision record (the fields of MaskedPhonemeDataset.decisions that collate_decisions packs). crop: crop_start > 0,
    n - crop_start > S, a masked word across the start of the window and a replaced one across its end; all: S ids, every
    position in a masked or replaced word; none: only action 0; gone: the crop removes the whole sample; short: n < S."""
    start = 0
    if kind == "crop":
        start = int(rs.randint(3, 40))
        n = start + S + int(rs.randint(3, 30))
    elif kind == "gone":
        n = int(rs.randint(1, S + 1))
        start = n + (0 if rs.randint(2) else 3)
    elif kind == "short":
        n = max(1, S - 1 - int(rs.randint(0, max(S // 2, 1))))
    else:
        n = S
    sep = rs.rand(n) < 0.2
    if kind == "all":
        sep[:] = False
    if kind == "crop":
        sep[start - 2:start + 2] = False
        sep[start + S - 2:start + S + 2] = False
    begin, length = [], []
    i = 0
    while i < n:
        if sep[i]:
            i += 1
            continue
        j = i
        cap = int(rs.randint(1, 8))
        while j < n and not sep[j] and j - i < cap:
            j += 1
        if kind == "crop":                       # the two straddling words stay whole
            for edge in (start, start + S):
                if i < edge < j + 1 and j < min(edge + 2, n):
                    j = min(edge + 2, n)
        begin.append(i)
        length.append(j - i)
        i = j
    begin, length = np.asarray(begin, np.int32), np.asarray(length, np.int32)
    if kind == "all":
        action = 1 + (np.arange(len(begin)) % 2)
    elif kind == "none":
        action = np.zeros(len(begin), np.int64)
    else:
        action = rs.randint(0, 3, size=len(begin))
    if kind == "crop":
        ends = begin + length
        action[(begin < start) & (ends > start)] = 1
        action[(begin < start + S) & (ends > start + S)] = 2
    return dict(ids=rs.randint(1, 187, size=n).astype(np.int64), repl=rs.randint(1000, 2000, size=n).astype(np.int64),
                word_begin=begin, word_len=length, action=action.astype(np.int8), crop_start=start, n=n,
                word_token=rs.randint(5000, 9000, size=len(begin)).astype(np.int64) if with_tok else None)


def _collate(recs, with_tok):
    """The flat layout of plbert_amd.data.collate_decisions (without its sort: the kernel does not need one)."""
    B = len(recs)
    sample_off, word_off = np.zeros(B + 1, np.int32), np.zeros(B + 1, np.int32)
    for b, r in enumerate(recs):
        sample_off[b + 1] = sample_off[b] + r["n"]
        word_off[b + 1] = word_off[b] + len(r["word_begin"])
    cat = lambda key, dt: np.concatenate([np.asarray(r[key], dtype=dt) for r in recs])   # noqa: E731
    return dict(ids=cat("ids", np.int64), repl=cat("repl", np.int64), sample_off=sample_off, word_off=word_off,
                word_begin=cat("word_begin", np.int32), word_len=cat("word_len", np.int32), action=cat("action", np.int8),
                crop_start=np.asarray([r["crop_start"] for r in recs], np.int32),
                word_token=cat("word_token", np.int64) if with_tok else None)


def _apply_args(d, B, S, with_tok, sep_token=87):
    ins = {k: _dev(d[k], dt) for k, dt in (("ids", np.int64), ("repl", np.int64), ("sample_off", np.int32), ("word_off", np.int32),
                                          ("word_begin", np.int32), ("word_len", np.int32), ("action", np.int8),
                                          ("crop_start", np.int32))}
    if with_tok:
        ins["word_token"] = _dev(d["word_token"], np.int64)
    Bo, So = max(B, 1), max(min(S, 1024), 1)
    outs = dict(labels=Out(Bo * So, torch.int64), masked=Out(Bo * So, torch.int64), tokens=Out(Bo * So, torch.int64),
                lengths=Out(Bo, torch.int32), counts=Out(Bo, torch.int32), idx=Out(Bo * So, torch.int32),
                offsets=Out(Bo + 3, torch.int32), flat=Out(Bo * So, torch.int32))
    p = _lib.PlbApplyMask()
    for k in ("ids", "sample_off", "word_off", "word_begin", "word_len", "action", "repl", "crop_start"):
        setattr(p, k, ins[k].data_ptr())
    p.word_token = ins["word_token"].data_ptr() if with_tok else None
    p.sep_token, p.B, p.S, p.mask_id = sep_token, B, S, mr.MASK_ID
    p.labels, p.masked, p.tokens = outs["labels"].ptr, outs["masked"].ptr, outs["tokens"].ptr if with_tok else None
    p.lengths_out, p.counts, p.idx_padded, p.offsets, p.flat = (outs[k].ptr for k in ("lengths", "counts", "idx", "offsets", "flat"))
    return p, ins, outs


def _run_apply(what, recs, S, with_tok):
    B = len(recs)
    d = _collate(recs, with_tok)
    p, ins, outs = _apply_args(d, B, S, with_tok)
    rc = _lib.lib().plb_launch_apply_mask(C.byref(p), stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    want = mr.apply_mask(d, S, mask_id=mr.MASK_ID, sep_token=87)
    for name in ("labels", "masked") + (("tokens",) if with_tok else ()):
        got = outs[name].get((B, S))
        if not np.array_equal(got, want[name]):
            b, i = (int(x) for x in np.argwhere(got != want[name])[0])
            raise AssertionError(f"{what}: {name}[{b}, {i}] is {int(got[b, i])}, the restatement has {int(want[name][b, i])}; "
                                 f"{int((got != want[name]).sum())} positions differ")
        assert outs[name].pads_ok(), f"{what}: a pad of {name} was written"
    if not with_tok:
        assert outs["tokens"].untouched()
    assert np.array_equal(outs["lengths"].get(), want["lengths"]) and outs["lengths"].pads_ok(), f"{what}: lengths_out"
    _check_csr(what, B, S, want["lists"], outs["counts"], outs["idx"], outs["offsets"], outs["flat"])
    return want


@pytest.mark.parametrize("with_tok", [False, True])
@pytest.mark.parametrize("S", [1, 255, 256, 257, 1000, 1024])
def test_apply_mask_equals_the_restatement(S, with_tok):
    rs = np.random.RandomState(1000 + S)
    recs = [_sample(kind, S, rs, with_tok) for kind in KINDS]
    want = _run_apply(f"S={S} B=5 tokens={with_tok}", recs, S, with_tok)
    crop, full, none, gone, short = range(5)
    assert want["lengths"].tolist()[:4] == [S, S, S, 0] and 0 < want["lengths"][short] < max(S, 2)
    assert np.array_equal(want["lists"][full], np.arange(S)) and len(want["lists"][none]) == 0 and len(want["lists"][gone]) == 0
    assert not want["labels"][gone].any() and not want["masked"][gone].any()
    assert want["lists"][crop][0] == 0 and want["lists"][crop][-1] == S - 1      # both straddling words reach into the window
    assert want["masked"][crop][S - 1] >= 1000 and (S < 8 or want["masked"][crop][0] == mr.MASK_ID)   # repl is 1000..1999
    if with_tok:
        assert (S < 8 or (want["tokens"][none] >= 5000).any()) and not want["tokens"][gone].any()   # action 0 writes its token
    for b, r in enumerate(recs):                                                  # B = 1: every kind alone
        _run_apply(f"S={S} B=1 kind={KINDS[b]} tokens={with_tok}", [r], S, with_tok)


@pytest.mark.parametrize("with_tok", [False, True])
def test_apply_mask_on_1024_samples(with_tok):
    rs = np.random.RandomState(5)
    recs = [_sample(KINDS[b % 5], 16, rs, with_tok) for b in range(1024)]
    want = _run_apply(f"S=16 B=1024 tokens={with_tok}", recs, 16, with_tok)
    assert sum(1 for x in want["lists"] if len(x)) > 500


@pytest.mark.parametrize("B,S", [(1, 0), (1, 1025), (0, 16), (1025, 16)])
def test_apply_mask_refusals_write_nothing(B, S):
    rs = np.random.RandomState(2)
    d = _collate([_sample("short", 16, rs, True)], True)
    p, ins, outs = _apply_args(d, B, S, True)
    assert _lib.lib().plb_launch_apply_mask(C.byref(p), stream()) != 0
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs.values())
