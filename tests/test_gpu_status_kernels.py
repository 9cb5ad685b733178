"""The status-word kernels and add_scalar (-m gpu): one-thread kernels whose clamping and merging rules decide whether a
data-parallel step reaches the parameters. Each launch is one row of a truth table; every buffer is a device word (the
host mirror too: the kernel only stores to it), written by the test — no fault is injected anywhere.

step_status_kernel: e = *ln_err; with `summed` (the ranks' counts after their all-reduce) f > 0.5 gives g = f < 2^20 ?
(unsigned)(f + 0.5) : 2^20, and g > e raises the word; the mirror gets e; a non-zero e turns the loss into NaN.
status_export_kernel: min(e, 2^20) as a float. add_scalar_kernel: out[0] = a[0] + b[0] in fp32."""
import math
import struct

import numpy as np
import pytest
import torch

from gpu_util import stream
from plbert_amd import _lib

pytestmark = pytest.mark.gpu

CAP = 1 << 20
LOSS = 2.71828
SENT = 0x5A5A5A5A
NAN = float("nan")


def _word(x):
    return torch.tensor([x - (1 << 32) if x >= 1 << 31 else x, SENT], dtype=torch.int32, device="cuda")   # [the word, a guard]


def _get(t):
    return int(t[0].item()) & 0xFFFFFFFF


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _f32bits(t):
    return int(t[:1].view(torch.int32).item()) & 0xFFFFFFFF


# (e at the start, summed or None) -> the word afterwards
STEP_CASES = [
    (0, None, 0),
    (3, None, 3),
    (0, 0.4, 0),                     # below 0.5: ignored
    (0, 0.5, 0),                     # f > 0.5 is strict
    (0, 2.0, 2),
    (0, 0.75, 1),                    # rounds to nearest
    (0, 2.5, 3),
    (5, 1.0, 5),                     # g > e only: a smaller sum never lowers the word
    (5, 5.0, 5),
    (5, 6.0, 6),
    (0, 3e6, CAP),
    (0, 1048575.0, CAP - 1),
    (0, 1048576.0, CAP),
    (0, float("inf"), CAP),
    (CAP + 5, 3e6, CAP + 5),         # the word itself is not clamped here
    (0, NAN, 0),                     # NaN > 0.5f is false: a NaN sum is ignored, the word stays
    (4, NAN, 4),
    (0, -7.0, 0),
]


@pytest.mark.parametrize("with_mirror", [True, False])
@pytest.mark.parametrize("with_loss", [True, False])
@pytest.mark.parametrize("e,summed,want", STEP_CASES)
def test_step_status_truth_table(e, summed, want, with_loss, with_mirror):
    L = _lib.lib()
    word, mirror = _word(e), _word(0xDEAD)
    loss = torch.tensor([LOSS, 1.5], dtype=torch.float32, device="cuda")
    sm = torch.tensor([summed, 9.0], dtype=torch.float32, device="cuda") if summed is not None else None
    sm_bits = _f32bits(sm) if sm is not None else None
    rc = L.plb_launch_step_status(word.data_ptr(), loss.data_ptr() if with_loss else None,
                                  mirror.data_ptr() if with_mirror else None, sm.data_ptr() if sm is not None else None, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert _get(word) == want and _get(word[1:]) == SENT
    assert _get(mirror) == (want if with_mirror else 0xDEAD) and _get(mirror[1:]) == SENT
    if with_loss and want:
        assert math.isnan(float(loss[0]))
    else:
        assert _f32bits(loss) == _bits(LOSS)                # bit-unchanged
    assert float(loss[1]) == 1.5
    if sm is not None:
        assert _f32bits(sm) == sm_bits and float(sm[1]) == 9.0


@pytest.mark.parametrize("e", [0, 1, CAP - 1, CAP, CAP + 1, (1 << 32) - 1])
def test_status_export_clamps_at_two_to_the_twenty(e):
    L = _lib.lib()
    word = _word(e)
    out = torch.tensor([-1.0, 7.0], dtype=torch.float32, device="cuda")
    assert L.plb_launch_status_export(word.data_ptr(), out.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [float(min(e, CAP)), 7.0]        # exact: every count up to 2^20 is an fp32 number
    assert _get(word) == e and _get(word[1:]) == SENT


def test_export_then_merge_carries_another_ranks_word():
    """The two kernels as engine_comm.cpp chains them: this rank's word 0 and another's 3 sum to 3.0; merged back, this rank
    skips too. Two ranks at the cap sum to 2^21: the merge clamps it to 2^20."""
    L = _lib.lib()
    for mine, other, want in ((0, 3, 3), (2, 0, 2), (CAP + 9, CAP, CAP + 9), (7, (1 << 32) - 1, CAP)):
        a, b = _word(mine), _word(other)
        fa, fb = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
        assert L.plb_launch_status_export(a.data_ptr(), fa.data_ptr(), stream()) == 0
        assert L.plb_launch_status_export(b.data_ptr(), fb.data_ptr(), stream()) == 0
        assert L.plb_launch_add_scalar(fa.data_ptr(), fa.data_ptr(), fb.data_ptr(), stream()) == 0    # the all-reduce
        loss = torch.tensor([LOSS], device="cuda")
        assert L.plb_launch_step_status(a.data_ptr(), loss.data_ptr(), None, fa.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        assert float(fa[0]) == float(min(mine, CAP) + min(other, CAP))
        assert _get(a) == max(mine, min(min(mine, CAP) + min(other, CAP), CAP)) == want and math.isnan(float(loss[0]))


ADD_CASES = [(1.0, 2.0), (0.1, 0.2), (16777216.0, 1.0), (1e-30, -1e-30), (3.4e38, 3.4e38), (float("inf"), 1.0),
             (float("inf"), float("-inf")), (NAN, 1.0), (1.0, NAN), (-0.0, 0.0), (-0.0, -0.0), (1.0000001, -1.0), (5.5, 0.0)]


@pytest.mark.parametrize("alias", ["none", "a", "b"])
@pytest.mark.parametrize("a,b", ADD_CASES)
def test_add_scalar_is_the_fp32_sum_bit_for_bit(a, b, alias):
    """out aliasing a is how engine_calls.cpp calls it (loss = loss + token loss)."""
    L = _lib.lib()
    ta = torch.tensor([a, 11.0], dtype=torch.float32, device="cuda")
    tb = torch.tensor([b, 12.0], dtype=torch.float32, device="cuda")
    to = {"none": torch.tensor([-5.0, 13.0], dtype=torch.float32, device="cuda"), "a": ta, "b": tb}[alias]
    a_bits, b_bits = _f32bits(ta), _f32bits(tb)
    assert L.plb_launch_add_scalar(to.data_ptr(), ta.data_ptr(), tb.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        want = np.float32(a) + np.float32(b)
    if np.isnan(want):
        assert math.isnan(float(to[0]))
    else:
        assert _f32bits(to) == _bits(float(want)), (float(to[0]), float(want))
    assert [float(ta[1]), float(tb[1])] == [11.0, 12.0] and (alias != "none" or float(to[1]) == 13.0)
    if alias != "a":
        assert _f32bits(ta) == a_bits
    if alias != "b":
        assert _f32bits(tb) == b_bits
