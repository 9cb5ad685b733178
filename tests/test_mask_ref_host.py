"""tests/mask_ref.py proved on the CPU (no GPU): the restatement tests/test_gpu_mask_kernels.py holds mask_words_kernel to.

 - Philox4x32-10 reproduces the published known-answer vectors (Random123's kat_vectors).
 - The restatement keeps the structural invariants tests/test_gpu_device_mask.py asserts of the kernel.
 - Its decisions have the distribution of dataloader.py:83-108, over 96360 words under four (seed, step) pairs that
   exercise both key halves and a full 32-bit step; the run is deterministic."""
import numpy as np
import pytest

import mask_ref as mr

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]
PAIRS = ((1234, 7), (2 ** 40 + 99, 0), (3, 2 ** 32 - 1), (0xDEADBEEFCAFEF00D, 123456))


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = mr.philox4x32_10(counter, key)
    assert tuple(int(x) for x in got) == want
    # vectorised: the same answer at every element of an array counter
    arr = mr.philox4x32_10(tuple(np.full(5, c, dtype=np.uint64) for c in counter), key)
    assert all((a == w).all() for a, w in zip(arr, want))


def test_u01_is_the_top_24_bits():
    x = np.array([0, 0xFF, 0x100, 0xFFFFFFFF, 0x80000000], dtype=np.uint64)
    u = mr.u01(x)
    assert u.dtype == np.float32 and u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5]


@pytest.fixture(scope="module")
def batch():
    return mr.random_labels(256, 512, 5)


@pytest.fixture(scope="module")
def runs(batch):
    lab, lengths = batch
    return [mr.mask_words(lab, lengths, seed, step) for seed, step in PAIRS]


def test_structure(batch, runs):
    lab, lengths = batch
    B, S = lab.shape
    for msk, lists in runs:
        for b in range(B):
            L, idx = lengths[b], lists[b]
            assert idx.dtype == np.int32 and (np.diff(idx) > 0).all() and (idx < L).all()    # ascending, inside the length
            assert (lab[b, idx] != mr.SEP_ID).all()                                          # separators never indexed
            keep = np.ones(S, bool)
            keep[idx] = False
            assert np.array_equal(msk[b, keep], lab[b, keep])                                # untouched outside the list
            pool = set(lab[b, :L][lab[b, :L] != mr.SEP_ID].tolist())
            iset = set(idx.tolist())
            for s, e in mr.words_of(lab[b], L):
                inside = [i in iset for i in range(s, e)]
                assert all(inside) or not any(inside)                                        # whole words
                if inside[0] and not (msk[b, s:e] == mr.MASK_ID).all():
                    assert set(msk[b, s:e].tolist()) <= pool                                 # replacements from the sample


def test_the_pairs_differ_from_each_other(batch, runs):
    """Every key half and every counter word is live: no two of the four runs agree, a run with the high key word cleared
    or the step truncated to 16 bits is another run."""
    lab, lengths = batch
    for i in range(4):
        for j in range(i + 1, 4):
            assert not np.array_equal(runs[i][0], runs[j][0])
    sub = (lab[:8], lengths[:8])
    a = mr.mask_words(*sub, 2 ** 40 + 99, 0)[0]
    assert not np.array_equal(a, mr.mask_words(*sub, 99, 0)[0])
    b = mr.mask_words(*sub, 3, 2 ** 32 - 1)[0]
    assert not np.array_equal(b, mr.mask_words(*sub, 3, 2 ** 16 - 1)[0])
    assert np.array_equal(b, mr.mask_words(*sub, 3, 2 ** 32 - 1)[0])


def test_statistics(batch, runs):
    lab, lengths = batch
    B, S = lab.shape
    words = [mr.words_of(lab[b], lengths[b]) for b in range(B)]
    assert sum(len(w) for w in words) == 24090
    n_words = n_sel = n_mask = n_repl = 0
    draws = []
    for (seed, step), (msk, lists) in zip(PAIRS, runs):
        key = (seed & mr.MASK32, seed >> 32)
        for b in range(B):
            # the decision of every word from its own counter: selection is not visible in the output when the word is kept
            r = mr.philox4x32_10((np.arange(len(words[b])), b, step & mr.MASK32, 0), key)
            n_words += len(words[b])
            sel = mr.u01(r[0]) < np.float32(0.15)
            n_sel += int(sel.sum())
            iset = set(lists[b].tolist())
            npool = int(((lab[b, :lengths[b]] != mr.SEP_ID)).sum())
            for k, (s, e) in enumerate(words[b]):
                if s in iset:
                    assert sel[k]
                    if (msk[b, s:e] == mr.MASK_ID).all() and mr.u01(r[1][k]) < np.float32(0.8):
                        n_mask += 1
                    else:
                        n_repl += 1
                        c = mr.philox4x32_10((np.arange(s, e), b, step & mr.MASK32, 1), key)
                        draws.extend((mr.u01(c[0]).astype(np.float64)).tolist())
                        assert npool > 0
    assert n_words == 96360
    z = lambda k, n, p: (k - n * p) / np.sqrt(n * p * (1 - p))   # noqa: E731
    z_sel, z_mask, z_repl = z(n_sel, n_words, 0.15), z(n_mask, n_sel, 0.8), z(n_repl, n_sel, 0.1)
    hist = np.histogram(np.asarray(draws), bins=16, range=(0.0, 1.0))[0]
    chi2 = float(((hist - len(draws) / 16) ** 2 / (len(draws) / 16)).sum())
    print(f"words {n_words} selected {n_sel} masked {n_mask} replaced {n_repl} draws {len(draws)}: "
          f"z {z_sel:.2f} {z_mask:.2f} {z_repl:.2f} chi2 {chi2:.1f}")
    assert abs(z_sel) <= 4 and abs(z_mask) <= 4 and abs(z_repl) <= 4
    assert chi2 <= 37.7                                           # the 99.9 % point at 15 degrees of freedom


def test_edges_of_the_decision_tree():
    lab, lengths = mr.random_labels(6, 100, 2)
    every = mr.mask_words(lab, lengths, 9, 1, probs=(1.0, 0.5, 0.5))[1]
    for b in range(6):
        want = np.flatnonzero((lab[b, :lengths[b]] != mr.SEP_ID))
        assert np.array_equal(every[b], want)                                  # every word changed: every phoneme indexed
    msk, lists = mr.mask_words(lab, lengths, 9, 1, probs=(1.0, 0.0, 1.0))
    assert not (msk == mr.MASK_ID).any() and sum(len(x) for x in lists) > 0     # everything replaced, nothing masked
    msk, lists = mr.mask_words(lab, lengths, 9, 1, probs=(0.0, 0.8, 0.1))
    assert np.array_equal(msk, lab) and all(len(x) == 0 for x in lists)
    counts, offsets, flat = mr.csr(every)
    assert offsets[0] == 0 and offsets[-1] == len(flat) == counts.sum() and offsets.dtype == flat.dtype == np.int32
    # garbage past the length is copied through and never indexed; lengths are clamped to [0, S]
    lab[0, lengths[0]:] = 77
    msk, lists = mr.mask_words(lab, [lengths[0], 0, -3, 1, 1000, 99], 9, 1)
    assert (msk[0, lengths[0]:] == 77).all() and len(lists[1]) == len(lists[2]) == 0 and (lists[4] < 100).all()


def test_apply_mask_restatement_on_a_hand_case():
    """One sample of 10 ids, crop_start 2, S = 6: the window is ids[2:8]. A masked word straddles the window's start, a
    replaced one its end, a kept one (action 0) lies inside and only writes its token."""
    d = dict(ids=np.arange(100, 110), repl=np.arange(200, 210), sample_off=np.array([0, 10], np.int32),
             word_off=np.array([0, 3], np.int32), word_begin=np.array([0, 4, 6], np.int32), word_len=np.array([3, 1, 4], np.int32),
             action=np.array([1, 0, 2], np.int8), crop_start=np.array([2], np.int32), word_token=np.array([11, 12, 13]))
    out = mr.apply_mask(d, 6, mask_id=185, sep_token=5)
    assert out["labels"].tolist() == [[102, 103, 104, 105, 106, 107]]
    assert out["masked"].tolist() == [[185, 103, 104, 105, 206, 207]]
    assert out["tokens"].tolist() == [[11, 5, 12, 5, 13, 13]]
    assert out["lengths"].tolist() == [6] and out["lists"][0].tolist() == [0, 4, 5]
    d["crop_start"] = np.array([12], np.int32)              # the crop removes the whole sample
    out = mr.apply_mask(d, 6, mask_id=185, sep_token=5)
    assert out["lengths"].tolist() == [0] and not out["labels"].any() and not out["tokens"].any() and len(out["lists"][0]) == 0
