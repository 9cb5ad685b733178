"""AdamW parameter groups on the CPU: plb_adamw_plan on a created, never bound engine (segment bounds, merging, holes, the
liveness rule, every scalar against the same double expression rounded once, every refusal) and the pure name resolution
of plbert_amd.train (resolve_param_groups, name_param_groups). Engine of tests/test_gpu_adamw_kernel.py: embedding 64, hidden
128, 2 heads, FFN 256, 2 layers, max_batch 2, max_seq 32; num_tokens 0 and 64.
The token head's step count (plb_token_head_steps + 1 in its segments) cannot be shown here: on a never bound engine no
dual-head call has run, the token head has no gradient and the plan omits it — which is what these tests show. The count
itself is asserted on the GPU, after a dual-head call (tests/test_gpu_adamw_groups.py, the "dual" case)."""
import ctypes as C

import numpy as np
import pytest
import torch

import plbert_amd
from plbert_amd import _lib
from plbert_amd import train as T

NAMES = _lib.PLB_PARAM_NAMES
IDX = {n: i for i, n in enumerate(NAMES)}
POOLER = ("encoder.pooler.weight", "encoder.pooler.bias")
HEAD = ("phoneme_predictor.weight", "phoneme_predictor.bias")
TOKEN = ("token_predictor.weight", "token_predictor.bias")
SCALARS = ("decay", "omb1", "b2", "omb2", "eps", "step_size", "bc2_sqrt")
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),
          dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
          dict(lr=1e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)]


class Created:
    """plb_create without a device: the handle and the flat layout."""

    def __init__(self, num_tokens=0, inference_only=0):
        self.L = _lib.lib()
        c = _lib.PlbConfig(188, 64, 128, 2, 256, 2, 512, 2, 1e-12, 188, num_tokens, 2, 32, inference_only)
        self.h = C.c_void_p()
        assert self.L.plb_create(C.byref(c), C.byref(self.h)) == 0
        offs, sizes = (C.c_int64 * _lib.PLB_NPARAM)(), (C.c_int64 * _lib.PLB_NPARAM)()
        total, train = C.c_int64(), C.c_int64()
        assert self.L.plb_param_layout(self.h, offs, sizes, C.byref(total), C.byref(train)) == 0
        self.off, self.size, self.total, self.train = list(offs), list(sizes), total.value, train.value

    def __del__(self):
        self.L.plb_destroy(self.h)

    def plan(self, groups, group_of, step, expect=0):
        garr = (_lib.PlbAdamWGroup * max(1, len(groups)))()
        for k, g in enumerate(groups):
            garr[k] = _lib.PlbAdamWGroup(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])
        gof = (C.c_int32 * _lib.PLB_NPARAM)(*group_of)
        segs = (_lib.PlbAdamWSegment * _lib.PLB_NPARAM)()
        n = C.c_int32(-1)
        rc = self.L.plb_adamw_plan(self.h, garr, len(groups), gof, step, segs, C.byref(n))
        if expect:
            assert rc != 0
            return self.L.plb_last_error().decode()
        assert rc == 0, self.L.plb_last_error()
        return [segs[i] for i in range(n.value)]


def _want_scalars(g, step):
    """The launcher's expressions (csrc/optim.hip: plb_launch_adamw) in Python doubles, rounded to fp32 once."""
    b1, b2 = g["betas"]
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return dict(decay=np.float32(1.0 - g["lr"] * g["weight_decay"]), omb1=np.float32(1.0 - b1), b2=np.float32(b2),
                omb2=np.float32(1.0 - b2), eps=np.float32(g["eps"]), step_size=np.float32(g["lr"] / bc1),
                bc2_sqrt=np.float32(np.sqrt(bc2)))


def _bits(x):
    return np.float32(x).view(np.uint32)


def _recipe(name):
    """The three groups of the torch comparison: embeddings | biases and LayerNorm | the rest; position table frozen."""
    if "position_embeddings" in name:
        return -1
    if "embeddings." in name:
        return 2
    return 1 if ("bias" in name or "LayerNorm" in name or "layer_norm" in name) else 0


@pytest.mark.parametrize("num_tokens", [0, 64])
def test_one_group_is_one_segment_over_the_trainable_range(num_tokens):
    e = Created(num_tokens)
    for step in (1, 7, 100000):
        segs = e.plan(GROUPS[:1], [0] * _lib.PLB_NPARAM, step)
        # the pooler never steps; on a fresh engine the phoneme head is live and the token head (no dual-head call) is not
        assert [(s.begin, s.end, s.group, s.step) for s in segs] == [(0, e.train, 0, step)]
        for k, want in _want_scalars(GROUPS[0], step).items():
            assert _bits(getattr(segs[0], k)) == _bits(want), (k, step)
    assert e.train == e.off[IDX[POOLER[0]]] and e.total > e.train


@pytest.mark.parametrize("num_tokens", [0, 64])
def test_groups_cut_merge_and_leave_holes(num_tokens):
    e = Created(num_tokens)
    group_of = [_recipe(n) for n in NAMES]
    step = 10
    segs = e.plan(GROUPS, group_of, step)
    # the expected cut, from the layout alone: runs of adjacent live tensors of one group
    want, live = [], []
    for i, n in enumerate(NAMES):
        if e.size[i] == 0 or n in POOLER or n in TOKEN or group_of[i] < 0:
            continue
        live.append(i)
        if want and want[-1][1] == e.off[i] and want[-1][2] == group_of[i]:
            want[-1][1] = e.off[i] + e.size[i]
        else:
            want.append([e.off[i], e.off[i] + e.size[i], group_of[i]])
    assert [[s.begin, s.end, s.group] for s in segs] == want
    assert len(segs) < len(live)                                   # merging happened (Q/K/V weights, then their biases, ...)
    assert all(s.begin % 4 == 0 and s.end % 4 == 0 and s.begin < s.end and s.step == step for s in segs)
    assert all(a.end <= b.begin for a, b in zip(segs, segs[1:]))
    pos = IDX["encoder.embeddings.position_embeddings.weight"]
    hole = (e.off[pos], e.off[pos] + e.size[pos])
    assert all(s.end <= hole[0] or s.begin >= hole[1] for s in segs)           # the frozen table is a hole
    assert segs[0].end == hole[0] and segs[1].begin == hole[1]
    assert max(s.end for s in segs) == e.train                               # nothing of the pooler or the token head
    for s in segs:
        for k, v in _want_scalars(GROUPS[s.group], step).items():
            assert _bits(getattr(s, k)) == _bits(v), (s.group, k)
    # two groups with the same settings do not merge (the group index is part of a segment) ...
    same = e.plan([GROUPS[0], dict(GROUPS[0])], [i % 2 for i in range(_lib.PLB_NPARAM)], step)
    assert len(same) == len([i for i in range(_lib.PLB_NPARAM) if e.size[i] and NAMES[i] not in POOLER + TOKEN])
    # ... and freezing everything leaves no segment
    assert e.plan(GROUPS, [-1] * _lib.PLB_NPARAM, step) == []
    # a group given to the pooler or to the idle token head changes nothing
    assert len(e.plan(GROUPS[:1], [0] * _lib.PLB_NPARAM, step)) == 1


def test_every_refusal_has_a_text():
    e = Created(0)
    ok = [0] * _lib.PLB_NPARAM
    g = GROUPS[0]
    assert "n_groups" in e.plan([], ok, 1, expect=1)
    assert "group_of[3] = 1" in e.plan([g], [0, 0, 0, 1] + [0] * (_lib.PLB_NPARAM - 4), 1, expect=1)
    assert "group_of[0] = -2" in e.plan([g], [-2] + ok[1:], 1, expect=1)
    for key, bad, word in (("lr", -1e-3, "lr"), ("lr", float("inf"), "lr"), ("lr", float("nan"), "lr"),
                           ("eps", -1e-8, "eps"), ("eps", float("nan"), "eps")):
        assert word in e.plan([{**g, key: bad}], ok, 1, expect=1)
    for betas, word in (((1.0, 0.999), "beta1"), ((-0.1, 0.999), "beta1"), ((0.9, 1.0), "beta2"), ((0.9, float("nan")), "beta2")):
        assert word in e.plan([{**g, "betas": betas}], ok, 1, expect=1)
    assert "step counts from 1" in e.plan([g], ok, 0, expect=1)
    assert e.plan([{**g, "betas": (0.0, 0.0)}], ok, 1)                         # [0, 1) includes 0
    # the step entry on an engine without buffers, and both on an inference-only engine: before anything is launched
    L = e.L
    garr = (_lib.PlbAdamWGroup * 1)(_lib.PlbAdamWGroup(g["lr"], 0.9, 0.999, g["eps"], g["weight_decay"]))
    gof = (C.c_int32 * _lib.PLB_NPARAM)(*ok)
    assert L.plb_adamw_step_groups(e.h, garr, 1, gof, 1, 1.0, None, None) != 0
    assert b"not bound" in L.plb_last_error()
    inf = Created(0, inference_only=1)
    assert "inference-only" in inf.plan([g], ok, 1, expect=1)
    assert L.plb_adamw_step_groups(inf.h, garr, 1, gof, 1, 1.0, None, None) != 0
    assert L.plb_grad_norm_groups(inf.h, gof, 1.0, 0.0, None, None) != 0
    assert b"inference-only" in L.plb_last_error()
    assert L.plb_grad_norm_groups(e.h, gof, 1.0, 0.0, None, None) != 0         # no norm buffer, no gradient buffer


# ---- the name resolution of plbert_amd.train -------------------------------------------------------------------------------
def _cfg():
    return plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)


def _params(names):
    return [(n, torch.nn.Parameter(torch.zeros(1))) for n in names]


def _layout():
    return plbert_amd.param_shapes(_cfg(), 188)        # the state-dict names of a PhonemeOnlyModel, flat-buffer order


def test_two_group_recipe_on_the_real_names():
    layout = _layout()
    assert list(layout) == [n for n in NAMES if n not in TOKEN]
    named = _params(layout)
    no_decay = [p for n, p in named if "bias" in n or "LayerNorm" in n]
    decay = [p for n, p in named if not ("bias" in n or "LayerNorm" in n)]
    group_of, frozen = T.resolve_param_groups(layout, named, [{"params": decay, "weight_decay": 0.01},
                                                             {"params": no_decay, "weight_decay": 0.0}])
    assert frozen == [] and set(group_of) == set(layout)
    assert group_of["encoder.embeddings.LayerNorm.weight"] == 1 and group_of["phoneme_predictor.bias"] == 1
    assert group_of["encoder.embeddings.word_embeddings.weight"] == 0
    layer = "encoder.encoder.albert_layer_groups.0.albert_layers.0."
    assert [group_of[layer + f"attention.{x}.weight"] for x in ("query", "key", "value")] == [0, 0, 0]
    assert group_of[layer + "ffn.bias"] == 1 and group_of[layer + "full_layer_layer_norm.weight"] == 0
    # the trainer's substring form gives the same membership
    groups = T.name_param_groups(layout, 0.01, ("bias", "LayerNorm"), ())
    assert [g["weight_decay"] for g in groups] == [0.01, 0.0]
    assert {n: k for k, g in enumerate(groups) for n in g["names"]} == group_of
    groups = T.name_param_groups(layout, 0.01, (), ("embeddings.",))
    assert len(groups) == 1 and not any("embeddings." in n for n in groups[0]["names"])
    assert len(groups[0]["names"]) == len(layout) - 5
    # "LayerNorm" alone misses full_layer_layer_norm; the documented recipe names it too
    full = T.name_param_groups(layout, 0.01, ("bias", "LayerNorm", "layer_norm"), ())
    assert layer + "full_layer_layer_norm.weight" in full[1]["names"] and layer + "ffn.weight" in full[0]["names"]
    # a frozen list that leaves nothing to train is refused where the groups are made
    with pytest.raises(ValueError, match="nothing would be trained"):
        T.name_param_groups(layout, 0.01, ("bias",), ("encoder", "predictor"))


def test_q_k_and_v_may_sit_in_different_groups():
    layout = _layout()
    named = _params(layout)
    q, k, v = ([p for n, p in named if f"attention.{x}.weight" in n] for x in ("query", "key", "value"))
    group_of, frozen = T.resolve_param_groups(layout, named, [{"params": q}, {"params": k}, {"params": v}])
    assert sorted(group_of.values()) == [0, 1, 2] and len(frozen) == len(layout) - 3


def test_duplicate_foreign_and_frozen_parameters():
    layout = _layout()
    named = _params(layout)
    ps = [p for _, p in named]
    with pytest.raises(ValueError, match="some parameters appear in more than one parameter group"):
        T.resolve_param_groups(layout, named, [{"params": ps[:3]}, {"params": ps[2:]}])
    with pytest.raises(ValueError, match="some parameters appear in more than one parameter group"):
        T.resolve_param_groups(layout, named, [{"params": [ps[0], ps[0]]}])
    with pytest.raises(ValueError, match="not one of the model's"):
        T.resolve_param_groups(layout, named, [{"params": ps + [torch.nn.Parameter(torch.zeros(1))]}])
    ps[1].requires_grad_(False)
    group_of, frozen = T.resolve_param_groups(layout, named, [{"params": ps[:4]}])
    assert frozen[0] == named[1][0] and named[1][0] not in group_of          # requires_grad == False, though in a group
    assert set(frozen) == {named[1][0]} | {n for n, _ in named[4:]}          # and everything that is in no group
    assert group_of == {named[0][0]: 0, named[2][0]: 0, named[3][0]: 0}
    one, _ = T.resolve_param_groups(layout, named, [{"params": ps[0]}])       # a bare tensor, as torch accepts it
    assert one == {named[0][0]: 0}


def test_a_stand_alone_albert_model_names_its_parameters_without_the_prefix():
    layout = _layout()
    bare = [n[len("encoder."):] for n in layout if n.startswith("encoder.")]
    named = _params(bare)
    group_of, frozen = T.resolve_param_groups(layout, named, [{"params": [p for _, p in named]}])
    assert frozen == [] and set(group_of) == {"encoder." + n for n in bare}
    assert "phoneme_predictor.weight" not in group_of
