"""AdamW per element (-m gpu): plb_launch_adamw and plb_launch_adamw_clipped against one step in float64 of the same fp32
inputs, within the allowance of gpu_util.adamw_fp64 (tests/test_adamw_elements_host.py proves the instrument on the CPU:
a float32 restatement of the kernel uses at most 0.54 / 0.25 / 0.62 of the p / m / v allowance, and every planted defect is
named). Ranges that end inside a workgroup, bias correction up to step 100000, the bf16 copy bit for bit, the skip word and
the non-finite flag as plain input words, the refusals, and sentinels around every buffer.

The kernel's worst share of each allowance on an MI355X (printed under -s), per range length over the 20 (lr, wd,
grad_scale) x step cases, and for the clipped form over its four:

    n        form            p      m      v
    4        plain           0.23   0.02   0.09
    1020     plain           0.31   0.23   0.38
    1024     plain           0.30   0.23   0.32
    1028     plain           0.31   0.23   0.35
    4100     plain           0.31   0.24   0.43
    262156   plain           0.31   0.25   0.42
    1028     clipped 1.0     0.30   0.23   0.35
    1028     clipped 0.37    0.29   0.22   0.44
    262156   clipped 1.0     0.31   0.25   0.42
    262156   clipped 0.37    0.31   0.25   0.62

(p sits below the restatement's 0.54 because the kernel forms p x decay - update as one fused operation.)
"""
import numpy as np
import pytest
import torch

import gpu_util as gu
from gpu_util import stream
from plbert_amd import _lib

pytestmark = pytest.mark.gpu

PAD, OFF = 64, 16                      # sentinel floats before and after; the range starts OFF floats behind the front pad
SENT_F32, SENT_BF16 = 0x7FC0ABCD, 0x7FC1   # NaN patterns no update produces
SIZES = (4, 1020, 1024, 1028, 4100, 262156)   # 1024 floats = one workgroup; 1028 = one workgroup and one thread; 257 workgroups
TRIPLES = gu.ADAMW_TRIPLES + (gu.ADAMW_DECAY_TRIPLE,)
HP = (gu.ADAMW_B1, gu.ADAMW_B2, gu.ADAMW_EPS)


class Range:
    """p, m, v, g (fp32) and the bf16 copy of one launch, each inside its own sentinel-filled buffer."""

    def __init__(self, state, with_bf16=True):
        self.n = n = state[0].shape[0]
        self.bufs = {}
        for name, a in zip("pgmv", state):
            buf = torch.full((PAD + OFF + n + PAD,), SENT_F32, dtype=torch.int32, device="cuda")
            buf[PAD + OFF:PAD + OFF + n] = torch.from_numpy(a.view(np.int32).copy()).cuda()
            self.bufs[name] = buf
        self.bufs["b"] = torch.full((PAD + OFF + n + PAD,), SENT_BF16, dtype=torch.int16, device="cuda")
        self.with_bf16 = with_bf16

    def ptr(self, name):
        if name == "b" and not self.with_bf16:
            return None
        buf = self.bufs[name]
        return buf.data_ptr() + (PAD + OFF) * buf.element_size()

    def args(self, lr, wd, gs, step, skip=None, count_skip=0):
        return (self.ptr("p"), self.ptr("g"), self.ptr("m"), self.ptr("v"), self.ptr("b"), self.n, lr, HP[0], HP[1], HP[2], wd,
                step, gs, skip.data_ptr() if skip is not None else None, count_skip)

    def get(self, name):
        a = self.bufs[name][PAD + OFF:PAD + OFF + self.n].cpu().numpy()
        return a.view(np.uint16) if name == "b" else a.view(np.float32)

    def assert_sentinels(self, what):
        for name, buf in self.bufs.items():
            s = SENT_BF16 if name == "b" else SENT_F32
            edge = torch.cat([buf[:PAD + OFF], buf[PAD + OFF + self.n:]])
            assert bool((edge == s).all()), f"{what}: the sentinels around {name} were written"

    def assert_untouched(self, state, what):
        for name, a in zip("pgmv", state):
            assert np.array_equal(self.get(name).view(np.uint32), a.view(np.uint32)), f"{what}: {name} was written"
        assert bool((self.bufs["b"] == SENT_BF16).all()), f"{what}: the bf16 copy was written"
        self.assert_sentinels(what)


def _launch(r, lr, wd, gs, step, skip=None, count_skip=0, norm=None, count_nonfinite=0):
    L = _lib.lib()
    a = r.args(lr, wd, gs, step, skip, count_skip)
    if norm is None:
        rc = L.plb_launch_adamw(*a, stream())
    else:
        rc = L.plb_launch_adamw_clipped(*a, norm.data_ptr(), count_nonfinite, stream())
    torch.cuda.synchronize()
    return rc


def _check(what, r, state, ref):
    p, m, v = r.get("p"), r.get("m"), r.get("v")
    ratios = gu.check_adamw(what, p, m, v, ref)
    assert np.array_equal(r.get("g").view(np.uint32), state[1].view(np.uint32)), f"{what}: the gradient was written"
    if r.with_bf16:
        gu.check_bf16_copy(what, r.get("b"), p)
    else:
        assert bool((r.bufs["b"] == SENT_BF16).all())
    r.assert_sentinels(what)
    return ratios


@pytest.mark.parametrize("n", SIZES)
def test_every_element_against_float64(n):
    state = gu.adamw_state(n)
    worst = {}
    for lr, wd, gs in TRIPLES:
        for step in gu.ADAMW_STEPS:
            ref = gu.adamw_fp64(*state, lr, wd, gs, step)
            r = Range(state)
            assert _launch(r, lr, wd, gs, step) == 0
            ratios = _check(f"n={n} lr={lr} wd={wd} gs={gs} step={step}", r, state, ref)
            for k, x in ratios.items():
                worst[k] = max(worst.get(k, 0.0), x)
    print(f"\nadamw n={n}: worst share of the allowance p {worst['p']:.2f} m {worst['m']:.2f} v {worst['v']:.2f}")


@pytest.mark.parametrize("coef", [1.0, 0.37])
@pytest.mark.parametrize("n", [1028, 262156])
def test_the_clipped_form(n, coef):
    state = gu.adamw_state(n)
    worst = {}
    for (lr, wd, gs), step in zip(TRIPLES, (1, 10, 100000, 2)):
        ref = gu.adamw_fp64(*state, lr, wd, gs, step, coef=np.float32(coef))
        r = Range(state)
        norm = torch.tensor([5.0, coef, 0.0, 2.0], dtype=torch.float32, device="cuda")
        assert _launch(r, lr, wd, gs, step, norm=norm, count_nonfinite=1) == 0
        ratios = _check(f"clipped n={n} coef={coef} lr={lr} step={step}", r, state, ref)
        assert norm.tolist() == [5.0, float(np.float32(coef)), 0.0, 2.0]         # a finite norm: nothing is counted
        for k, x in ratios.items():
            worst[k] = max(worst.get(k, 0.0), x)
    print(f"\nadamw clipped n={n} coef={coef}: worst share p {worst['p']:.2f} m {worst['m']:.2f} v {worst['v']:.2f}")


def test_the_nonfinite_flag_writes_nothing_and_counts_only_when_asked():
    state = gu.adamw_state(4100)
    r = Range(state)
    norm = torch.tensor([float("inf"), 0.0, 1.0, 2.0], dtype=torch.float32, device="cuda")
    lr, wd, gs = TRIPLES[1]
    assert _launch(r, lr, wd, gs, 3, norm=norm, count_nonfinite=1) == 0
    assert norm.tolist()[2:] == [1.0, 3.0]
    assert _launch(r, lr, wd, gs, 3, norm=norm, count_nonfinite=0) == 0
    assert norm.tolist()[2:] == [1.0, 3.0]
    assert _launch(r, lr, wd, gs, 3, norm=norm, count_nonfinite=1) == 0
    assert norm.tolist()[2:] == [1.0, 4.0]                    # one per launch (five workgroups ran)
    r.assert_untouched(state, "norm[2] != 0")


def test_the_bf16_copy_without_an_update_pins_the_tie_rule():
    """lr = 0, wd = 0: p x 1 - 0 x (m / den) leaves p bit-unchanged while m and v still move, so the copy is the rounding
    of values the test chose: exact ties towards the even neighbour below and above, both signs, and their neighbours."""
    ties = gu.bf16_tie_values()
    n = 1028
    p, g, m, v = gu.adamw_state(n)
    p = p.copy()
    p[:ties.size] = ties
    p[1024:1028] = ties[:4]                                    # and in the one thread of the second workgroup
    state = (p, g, m, v)
    r = Range(state)
    assert _launch(r, 0.0, 0.0, 1.0, 5) == 0
    assert np.array_equal(r.get("p").view(np.uint32), p.view(np.uint32))
    gu.check_bf16_copy("ties", r.get("b"), p)
    ref = gu.adamw_fp64(*state, 0.0, 0.0, 1.0, 5)
    gu.check_adamw("lr=0", r.get("p"), r.get("m"), r.get("v"), ref)
    moved = (r.get("m") != m) | (r.get("v") != v)
    assert int(moved.sum()) > n // 2
    r.assert_sentinels("ties")


@pytest.mark.parametrize("n", [1028, 4100])
def test_without_a_bf16_copy(n):
    state = gu.adamw_state(n)
    lr, wd, gs = TRIPLES[1]
    r = Range(state, with_bf16=False)
    assert _launch(r, lr, wd, gs, 10) == 0
    _check("p_bf16 = NULL", r, state, gu.adamw_fp64(*state, lr, wd, gs, 10))
    assert not np.array_equal(r.get("p"), state[0])


@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("count_skip", [0, 1, 2])
def test_the_skip_word(count_skip, clipped):
    """skip[0] != 0: nothing changes and skip[count_skip] grows by exactly 1 per launch — not once per workgroup (257 here);
    at count_skip 0 nothing is counted. The word is a plain input the test writes."""
    n = 262156
    state = gu.adamw_state(n)
    lr, wd, gs = TRIPLES[0]
    r = Range(state)
    norm = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float32, device="cuda") if clipped else None
    skip = torch.tensor([3, 10, 20, 30], dtype=torch.int32, device="cuda")
    for k in range(3):
        assert _launch(r, lr, wd, gs, 4, skip=skip, count_skip=count_skip, norm=norm, count_nonfinite=1) == 0
        want = [3, 10, 20, 30]
        if count_skip:
            want[count_skip] += k + 1
        assert skip.tolist() == want
    r.assert_untouched(state, "skip[0] != 0")
    if clipped:
        assert norm.tolist() == [1.0, 1.0, 0.0, 0.0]
    # skip[0] == 0: the launch updates and counts nothing
    skip = torch.tensor([0, 10, 20, 30], dtype=torch.int32, device="cuda")
    assert _launch(r, lr, wd, gs, 4, skip=skip, count_skip=count_skip, norm=norm) == 0
    _check("skip[0] == 0", r, state, gu.adamw_fp64(*state, lr, wd, gs, 4, coef=np.float32(1.0) if clipped else None))
    assert skip.tolist() == [0, 10, 20, 30]


def test_refusals_write_nothing():
    L = _lib.lib()
    state = gu.adamw_state(1028)
    lr, wd, gs = TRIPLES[0]
    r = Range(state)
    norm = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    for n, step in ((1027, 1), (1026, 1), (2, 1), (1028, 0), (1028, -1)):
        a = list(r.args(lr, wd, gs, step))
        a[5] = n
        assert L.plb_launch_adamw(*a, stream()) != 0
        assert L.plb_launch_adamw_clipped(*a, norm.data_ptr(), 1, stream()) != 0
    a = list(r.args(lr, wd, gs, 1))
    assert L.plb_launch_adamw_clipped(*a, None, 0, stream()) != 0          # the clipped form needs its norm buffer
    a[5] = 0
    assert L.plb_launch_adamw(*a, stream()) == 0                            # an empty range is not an error
    assert L.plb_launch_adamw_clipped(*a, norm.data_ptr(), 1, stream()) == 0
    torch.cuda.synchronize()
    r.assert_untouched(state, "refused")
    assert norm.tolist() == [1.0, 1.0, 0.0, 0.0]
