"""The slice contract of tests/grad_slices_ref.py on the CPU, on the small case of tests/test_gpu_grad_slices.py: the
variants of the rounding model pass it against each other, and every defect of DEFECTS — each of which the per-tensor
relative L2 of 4e-2 (test_gpu_engine._grad_close) passes — raises and is named by tensor, axis and slice. The stand-in for
the device is the float32 / pruned variant of the restatement.

Figures of the small case (deterministic; the test prints them under -s): loo 1.119, FACTOR 2.239.

    defect                                        per-tensor rel L2   err / scale   over FACTOR
    one row of ffn.weight's gradient zeroed       3.57e-02            88.3          39.4 x
    one ffn.bias element zeroed                   3.54e-02            10.5           4.7 x
    one word-embedding row x1.5                   2.67e-02            80.5          35.9 x
    one column of attention.dense.weight zeroed   3.46e-02            74.3          33.2 x
    one row of ffn.weight x1.1                    1.86e-02            18.9           8.4 x
    one position row below S doubled              1.07e-02            148.7         66.4 x
"""
import re

import numpy as np
import pytest

import grad_slices_ref as R


@pytest.fixture(scope="module")
def case():
    return R.build_case("small")


def test_slicing():
    v = dict(R.views(np.arange(12.0).reshape(3, 4)))
    assert v["row"].shape == (3, 4) and v["col"].shape == (4, 3) and v["col"][1].tolist() == [1.0, 5.0, 9.0]
    assert dict(R.views(np.zeros(128)))["block"].shape == (2, 64)
    assert dict(R.views(np.zeros(188)))["block"].shape == (1, 188)   # no multiple of 64: the whole tensor


def test_reference_is_the_oracle(case):
    """amax=None, bf16=False is albert_np.loss_and_grads (tests/test_oracle_fp8.py holds the equality in general)."""
    from oracle import albert_np
    loss, _, G = albert_np.loss_and_grads(case["ocfg"], case["sd"], case["masked"], case["labels"], case["lengths"], case["idx"],
                                          dtype=np.float64)
    assert abs(float(loss) - case["loss"]) <= 1e-12 * case["loss"]
    assert set(G) == set(case["ref"])
    for k, g in G.items():
        assert np.abs(g - case["ref"][k]).max() <= 1e-9 * np.abs(g).max() + 1e-15, k


def test_exact_zero_slices_are_the_ones_the_batch_predicts(case):
    ids = set(case["masked"].reshape(-1).tolist()) - {0}
    S, nz = case["spec"]["S"], case["nonzero"]
    word, pos, typ = (R.ENC + f"embeddings.{n}_embeddings.weight" for n in ("word", "position", "token_type"))
    assert sorted(np.flatnonzero(nz[word, "row"]).tolist()) == sorted(ids)          # absent ids and row 0: exactly zero
    assert nz[pos, "row"].tolist() == [i < S for i in range(512)]
    assert nz[typ, "row"].tolist() == [True, False]
    assert all(m.all() for (k, axis), m in nz.items() if (k, axis) not in ((word, "row"), (pos, "row"), (typ, "row")))
    assert case["zeros"][word] == 188 - len(ids) and case["zeros"][pos] == 512 - S and case["zeros"][typ] == 1


def test_each_variant_passes_against_the_other_three(case):
    assert case["factor"] == 2.0 * case["loo"]
    print(f"\nsmall: loo {case['loo']:.4f}, FACTOR {case['factor']:.4f}")
    for v, grads in case["variants"].items():
        st = R.check_slices(case, grads, scales=R.slice_scales(case, without=v))
        worst = max(s["ratio"] for s in st.values())
        assert worst == case["loo_by_variant"][v][0] <= case["loo"]
        print(f"  {v:10s} against the other three: worst err / scale {worst:.3f}")
    R.check_slices(case, case["variants"][R.STAND_IN])                             # and against the case's own scales


@pytest.mark.parametrize("what,inject,whole", R.DEFECTS, ids=[d[0].replace(" ", "-") for d in R.DEFECTS])
def test_defect_the_per_tensor_rule_passes_is_caught_and_named(case, what, inject, whole):
    G = {k: g.copy() for k, g in case["variants"][R.STAND_IN].items()}
    tensor, axis, i = inject(case, G)
    changed = [k for k in G if not np.array_equal(G[k], case["variants"][R.STAND_IN][k])]
    assert changed == [tensor]
    per_tensor = R.rel_l2(G[tensor], case["ref"][tensor])
    assert per_tensor < R.PER_TENSOR, (what, per_tensor)                            # the gap: _grad_close lets it through
    ratio = R.slice_errors(G, case["ref"])[tensor, axis][i] / case["scale"][tensor, axis][i]
    print(f"\n{what}: {axis} {i}, per-tensor rel L2 {per_tensor:.3e}, err / scale {ratio:.1f} = {ratio / case['factor']:.1f} x FACTOR")
    with pytest.raises(AssertionError, match=re.escape(f"{tensor}: {axis} {i} is off by")):
        R.check_slices(case, G)
    if whole:   # what keeps FACTOR honest: a whole-slice fault stands well clear of it
        assert ratio >= 1.5 * case["factor"], (what, ratio, case["factor"])


def test_zero_and_key_bias_rules(case):
    base = case["variants"][R.STAND_IN]
    word = R.ENC + "embeddings.word_embeddings.weight"
    G = dict(base, **{word: base[word].copy()})
    G[word][0, 3] = 1e-30                                                           # row 0: the padding id
    with pytest.raises(AssertionError, match=re.escape(f"{word}: row 0 has an exactly zero reference")):
        R.check_slices(case, G)
    G[word] = base[word].copy()
    G[word][int(np.flatnonzero(case["nonzero"][word, "row"])[0])] = 0.0            # a row that must NOT be zero
    with pytest.raises(AssertionError):
        R.check_slices(case, G)
    G = dict(base, **{R.KEY_BIAS: base[R.QUERY_BIAS] * 0.05})
    with pytest.raises(AssertionError, match="its true gradient is zero"):
        R.check_slices(case, G)
