"""Token-packed execution, host side (no GPU): the C ABI declares and exports the packed entry points, the host plan helper
lays ragged batches out correctly, and staging with packing on yields the padded tensors of before plus the plan."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
import plbert_amd
from plbert_amd import _lib
from plbert_amd.engine import PackingPlan, packing_plan

PACKED_SYMBOLS = ["plb_packing_plan", "plb_forward_packed", "plb_loss_fwd_bwd_packed", "plb_loss_fwd_packed",
                  "plb_last_call_rows"]


def rup(x, m):
    return (x + m - 1) // m * m


def test_library_exports_the_packed_entry_points():
    L = _lib.lib()
    for s in PACKED_SYMBOLS:
        assert s in _lib.PUBLIC_SYMBOLS and hasattr(L, s), s
    for s in ("plb_launch_ce_prepare_packed", "plb_launch_unpack_rows"):
        assert hasattr(L, s), s


def _check_plan(lengths, S):
    """Invariants of any plan: monotone 128-aligned starts, slots that do not overlap and hold every valid token exactly
    once, a row count that is a multiple of the granularity and never above the padded call's."""
    B = len(lengths)
    plan = packing_plan(lengths, S)
    rs = plan.row_start_host
    padded = rup(B * S, 128)
    # the chosen granularity: the coarsest of 1024 / 256 / 128 that still leaves fewer rows than the padded call
    gran = next((m for m in (1024, 256) if rup(int(rs[B]), m) < padded), 128)
    assert rs.shape == (B + 1,) and rs[0] == 0 and rs[B] == plan.used
    assert plan.rows % gran == 0 and plan.rows % 128 == 0 and plan.used <= plan.rows <= padded
    lens = np.clip(np.asarray(lengths), 1, S)
    owner = np.full(plan.rows, -1)
    for b in range(B):
        assert rs[b + 1] >= rs[b] + lens[b], (b, rs)           # monotone, the sample's tokens fit before the next start
        rows = np.arange(rs[b], rs[b] + lens[b])
        assert rows[-1] < plan.used and (owner[rows] == -1).all()  # inside the used rows, nobody else's
        owner[rows] = b
    assert (owner >= 0).sum() == lens.sum() == plan.valid_tokens
    if plan.packed:
        assert (rs % 128 == 0).all() and plan.rows < padded
        assert plan.used == sum(rup(int(x), 128) for x in lens) and plan.rows == rup(plan.used, gran)
    else:                                                       # nothing to gain: the plan is the padded layout
        assert plan.rows == padded and (rs == np.arange(B + 1) * S).all()
    return plan


def test_plan_of_the_ragged_fixture():
    g = load_golden("real_s512_b32_ragged")
    lengths = [int(x) for x in g["lengths"]]
    plan = _check_plan(lengths, 512)
    assert plan.packed and plan.valid_tokens == 10271
    assert plan.used == 12032 and plan.rows == 12288            # 128-aligned slots, rounded to the fused-LayerNorm multiple
    g2 = load_golden("real_s512_b2_ragged")
    plan2 = _check_plan([int(x) for x in g2["lengths"]], 512)
    assert plan2.packed and plan2.rows == 896                   # 512 + 384: only the 128-row granularity saves anything


@pytest.mark.parametrize("lengths,S,packed", [
    ([512] * 4, 512, False),                  # all full: the padded layout
    ([100], 640, True),                       # one sample
    ([300], 512, True),                       # 384 rows: only the 128-row granularity saves anything
    ([400], 512, False),                      # a sample that needs every tile of the padded call
    ([1], 640, True),                         # length 1
    ([300, 100, 50, 20], 512, True),
    ([1, 1, 1, 1], 512, True),
    ([500, 130, 129, 65, 63, 1], 512, True),  # lengths that are no multiples of 64
    ([96, 80, 50, 96], 96, False),            # S below the 128-row slot: packing would need MORE rows
    ([33, 32, 2, 1, 1], 33, False),
    ([65, 64, 63], 65, False),
    ([90, 77, 64, 13, 1], 90, False),
    ([512, 511], 512, False),                 # a last tile saved nowhere
    ([512, 384], 512, True),                  # 896 rows at the 128-row granularity
    ([512, 256, 256, 512, 128, 128, 128, 128], 512, True),
    ([0, 700], 512, True),                    # out-of-range lengths are clamped to [1, S], as the kernels clamp them
])
def test_plan_edge_cases(lengths, S, packed):
    assert _check_plan(lengths, S).packed == packed


def test_plan_rejects_bad_arguments():
    with pytest.raises(RuntimeError):
        PackingPlan([], 512)
    with pytest.raises(RuntimeError):
        PackingPlan([5], 0)


def test_staging_with_packing_on_keeps_the_padded_tensors_and_adds_the_plan(monkeypatch):
    from plbert_amd.train import stage_reference_batch
    g = load_golden("real_s512_b32_ragged")
    batch = (g["labels"], g["masked"], [int(x) for x in g["lengths"]], [list(map(int, x)) for x in g["index"]])
    eng = types.SimpleNamespace(device=torch.device("cpu"), cfg=types.SimpleNamespace(vocab_size=188), num_tokens=0)
    monkeypatch.delenv("PLBERT_PACKED", raising=False)
    plain = stage_reference_batch(eng, batch)
    packed = stage_reference_batch(eng, batch, packed=True)
    assert plain.packing is None and packed.packing is not None
    for f in ("masked", "labels", "lengths", "offsets", "flat"):
        assert torch.equal(getattr(plain, f), getattr(packed, f)), f
    assert (plain.n_masked, plain.n_tokens) == (packed.n_masked, packed.n_tokens)
    plan = packed.packing
    assert plan.packed and plan.rows == 12288 and plan.row_start.dtype == torch.int32
    assert np.array_equal(plan.row_start.numpy(), plan.row_start_host) and np.array_equal(packed.lengths_host, g["lengths"])
    monkeypatch.setenv("PLBERT_PACKED", "1")                    # the environment switch, in the style of the others
    assert stage_reference_batch(eng, batch).packing is not None
    assert stage_reference_batch(eng, batch, packed=False).packing is None
    # a batch without padding has nothing to pack
    full = (g["labels"], g["masked"], [512] * 32, [[1]] * 32)
    assert stage_reference_batch(eng, full, validate=False, packed=True).packing is None
