"""The bitwise difference reporter for gradient buffers (tests/gpu_util.py: first_difference) on the CPU: a fake parameter
layout, buffers that differ where the test put the difference. The reporter compares bit patterns; the cases below fail
for one that compared floats with == (a NaN of identical bits on both sides would differ) or with an absolute difference
(one unit in the last place would pass)."""
import struct
from types import SimpleNamespace

import pytest
import torch

from gpu_util import assert_same_bits, first_difference, format_difference

# three tensors and a gap of 5 elements no tensor covers (as the pooler between the heads of the real layout)
LAYOUT = SimpleNamespace(layout={"emb.weight": (0, 12, (3, 4)), "value.weight": (12, 30, (5, 6)),
                                 "head.bias": (47, 7, (7,))})
N = 54


def _buf(seed=0):
    return torch.randn(N, generator=torch.Generator().manual_seed(seed))


def _set_bits(t, i, bits):
    t.view(torch.int32)[i] = bits if bits < 2 ** 31 else bits - 2 ** 32


def test_equal_buffers():
    a = _buf()
    assert first_difference(LAYOUT, a, a.clone()) == []
    assert_same_bits(LAYOUT, a, a.clone(), "equal")


def test_one_element_of_the_last_tensor():
    a = _buf()
    b = a.clone()
    b[47 + 5] = 3.0
    (r,) = first_difference(LAYOUT, a, b)
    assert r["name"] == "head.bias" and r["count"] == 1 and r["index"] == [5]
    assert r["a"] == float(a[52]) and r["b"] == 3.0 and r["b_bits"] == 0x40400000
    assert r["a_bits"] == struct.unpack("<I", struct.pack("<f", float(a[52])))[0]
    with pytest.raises(AssertionError, match=r"after H1: 1 tensor differ — head\.bias: 1 element, first at \[5\]: .*0x40400000"):
        assert_same_bits(LAYOUT, a, b, "after H1")


def test_coordinates_counts_and_every_tensor_named():
    a = _buf()
    b = a.clone()
    for i in (12 + 3 * 6 + 2, 12 + 4 * 6 + 5, 2 * 4 + 1):          # value.weight [3, 2] and [4, 5], emb.weight [2, 1]
        b[i] += 1.0
    recs = first_difference(LAYOUT, a, b)
    assert [(r["name"], r["count"], r["index"]) for r in recs] == [("emb.weight", 1, [2, 1]), ("value.weight", 2, [3, 2])]
    text = format_difference(recs)
    assert "value.weight: 2 elements, first at [3, 2]" in text and "emb.weight: 1 element, first at [2, 1]" in text


def test_one_unit_in_the_last_place_is_a_difference():
    a = torch.ones(N)
    b = a.clone()
    _set_bits(b, 20, 0x3F800001)
    (r,) = first_difference(LAYOUT, a, b)
    assert (r["name"], r["index"], r["a_bits"], r["b_bits"]) == ("value.weight", [1, 2], 0x3F800000, 0x3F800001)


def test_signed_zeros_are_equal():
    """The one pair of different bit patterns that is NOT a difference (first_difference's docstring): +0 against -0."""
    a = _buf()
    a[13] = 0.0
    b = a.clone()
    _set_bits(b, 13, 0x80000000)
    assert float(b[13]) == 0.0 and int(b.view(torch.int32)[13]) != 0
    assert first_difference(LAYOUT, a, b) == [] and first_difference(LAYOUT, b, a) == []
    # ... but a zero against the smallest subnormal is one
    _set_bits(b, 13, 0x80000001)
    (r,) = first_difference(LAYOUT, a, b)
    assert (r["name"], r["index"], r["b_bits"]) == ("value.weight", [0, 1], 0x80000001)


def test_nan_of_identical_bits_is_equal_and_nan_against_a_number_is_not():
    a = _buf()
    b = a.clone()
    for t in (a, b):
        _set_bits(t, 30, 0x7FC00123)                               # the same quiet NaN, payload and all
    assert bool(torch.isnan(a[30])) and not bool(a[30] == b[30])   # what a float comparison says
    assert not torch.equal(a, b)
    assert first_difference(LAYOUT, a, b) == []
    b[30] = 1.5
    (r,) = first_difference(LAYOUT, a, b)
    assert (r["name"], r["count"], r["index"]) == ("value.weight", 1, [3, 0])
    assert r["a"] != r["a"] and r["b"] == 1.5 and r["a_bits"] == 0x7FC00123
    _set_bits(b, 30, 0xFFC00123)                                   # a NaN of other bits: not what the other engine wrote
    assert len(first_difference(LAYOUT, a, b)) == 1


def test_buffer_shorter_than_the_layout_and_elements_outside_it():
    a = _buf()
    b = a.clone()
    b[44] = 9.0                                                    # the gap between value.weight and head.bias
    (r,) = first_difference(LAYOUT, a, b)
    assert r["name"] == "(outside the layout)" and r["index"] == [44] and r["count"] == 1
    b = a.clone()
    b[41] = 9.0
    (r,) = first_difference(LAYOUT, a[:42], b[:42])                # grads[:trainable]: later tensors are simply absent
    assert (r["name"], r["index"]) == ("value.weight", [4, 5])
    b = a.clone()
    b[12 + 2 * 6 + 1] = 9.0
    (r,) = first_difference(LAYOUT, a[:30], b[:30])                # the buffer ends inside value.weight: still a coordinate
    assert (r["name"], r["index"]) == ("value.weight", [2, 1])
    with pytest.raises(ValueError):
        first_difference(LAYOUT, a, b[:10])
