"""LAMB on the CPU: the float64 restatement against its second form, plb_lamb_plan on a created, never bound engine, the
state dict of plbert_amd.train.Lamb over a stand-in engine, the new symbols in the library and the binding table, and the
default-path guarantee of PLBertTrainer. Engine of tests/test_adamw_groups_host.py: embedding 64, hidden 128, 2 heads, FFN 256,
2 layers, max_batch 2, max_seq 32; num_tokens 0 and 64.
The token head's own step count (plb_token_head_steps + 1 in its segments) cannot be shown on a never bound engine: no
dual-head call has run, so the token head has no gradient and the plan leaves it out — which is what is asserted here, with the
count set beforehand. The count in the plan is asserted on the GPU after a dual-head call (tests/test_gpu_lamb.py)."""
import ctypes as C
import fnmatch
import os
import re
import subprocess
from collections import OrderedDict

import numpy as np
import pytest
import torch

import c_header
import lamb_ref as R
import plbert_amd
from plbert_amd import _lib
from plbert_amd import train as T

NAMES = _lib.PLB_PARAM_NAMES
IDX = {n: i for i, n in enumerate(NAMES)}
POOLER = ("encoder.pooler.weight", "encoder.pooler.bias")
TOKEN = ("token_predictor.weight", "token_predictor.bias")
NEW_PUBLIC = ("plb_lamb_floats", "plb_lamb_plan", "plb_lamb_step")
NEW_INTERNAL = ("plb_lamb_workgroups", "plb_launch_lamb_pass1", "plb_launch_lamb_finish", "plb_launch_lamb_pass2")
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, adapt=1),
          dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.0, adapt=0)]


# ---- 1. the restatement against its second form ---------------------------------------------------------------------------
def test_the_two_forms_of_the_restatement_agree():
    rng = np.random.RandomState(3)
    bounds = ((0, 8), (8, 40), (44, 60), (60, 100), (100, 132))      # [40, 44) is a hole
    n = 136
    p, g, m = (rng.randn(n).astype(np.float32) for _ in range(3))
    v = (rng.randn(n).astype(np.float32) ** 2)
    p[8:40] = 0.0                                                     # wn = 0
    g[44:60] = 0.0; m[44:60] = 0.0; v[44:60] = 0.0                    # zero gradient, zero decay, zero moments: un = 0
    tensors = [R.tensor(a, b, lr=1e-3 * (k + 1), betas=((0.9, 0.999), (0.8, 0.99))[k % 2], eps=1e-6,
                        weight_decay=0.0 if k == 2 else 0.01, step=(1, 7, 3, 100, 2)[k], adapt=0 if k == 4 else 1, slot=k)
               for k, (a, b) in enumerate(bounds)]
    for gs, coef in ((1.0, None), (0.125, 0.37)):
        a, b = R.lamb_ref(p, g, m, v, tensors, gs, coef), R.lamb_ref_loop(p, g, m, v, tensors, gs, coef)
        for k in ("p", "m", "v", "u"):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-13, atol=1e-300, err_msg=k)
        for k in ("wn", "un", "trust"):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-13, err_msg=k)
        assert a["wn"][1] == 0.0 and a["trust"][1] == 1.0 and a["un"][1] > 0.0        # an all-zero tensor
        assert a["un"][2] == 0.0 and a["trust"][2] == 1.0 and a["wn"][2] > 0.0        # nothing to apply
        assert np.array_equal(a["p"][44:60], p[44:60].astype(np.float64))
        assert a["trust"][4] == 1.0 and a["wn"][4] > 0 and a["un"][4] > 0             # adapt = 0
        assert a["trust"][0] == a["wn"][0] / a["un"][0] != 1.0
        assert np.isfinite(a["p"]).all()
        for k, src in (("p", p), ("m", m), ("v", v)):                                   # the hole comes back unchanged
            assert np.array_equal(a[k][40:44], src[40:44].astype(np.float64)) and np.array_equal(a[k][132:], src[132:])
    # the scalars are rounded once from double expressions
    s = R.scalars(1e-3, (0.9, 0.999), 1e-6, 0.01, 7)
    assert s["inv_bc1"] == float(np.float32(1.0 / (1.0 - 0.9 ** 7))) and s["omb2"] == float(np.float32(1.0 - 0.999))


# ---- 2. plb_lamb_plan ------------------------------------------------------------------------------------------------------
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

    @staticmethod
    def groups_c(groups):
        garr = (_lib.PlbLambGroup * max(1, len(groups)))()
        for k, g in enumerate(groups):
            garr[k] = _lib.PlbLambGroup(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], g["adapt"])
        return garr

    def plan(self, groups, group_of, step, expect=0):
        gof = (C.c_int32 * _lib.PLB_NPARAM)(*group_of)
        segs = (_lib.PlbLambSegment * _lib.PLB_NPARAM)()
        n = C.c_int32(-1)
        rc = self.L.plb_lamb_plan(self.h, self.groups_c(groups), len(groups), gof, step, segs, C.byref(n))
        if expect:
            assert rc != 0
            return self.L.plb_last_error().decode()
        assert rc == 0, self.L.plb_last_error()
        return [segs[i] for i in range(n.value)]


def _bits(x):
    return np.float32(x).view(np.uint32)


@pytest.mark.parametrize("num_tokens", [0, 64])
def test_plan_has_one_segment_per_live_tensor_never_merged(num_tokens):
    e = Created(num_tokens)
    assert e.L.plb_set_token_head_steps(e.h, 41) == 0               # (its tensors have no gradient yet: they stay out)
    frozen = ("encoder.embeddings.position_embeddings.weight", "encoder.encoder.albert_layer_groups.0.albert_layers.0.ffn.bias")
    group_of = [-1 if n in frozen else (1 if "bias" in n or "LayerNorm" in n or "layer_norm" in n else 0) for n in NAMES]
    step = 10
    segs = e.plan(GROUPS, group_of, step)
    live = [i for i, n in enumerate(NAMES) if e.size[i] and n not in POOLER + TOKEN + frozen]
    assert [s.tensor for s in segs] == live                           # holes: frozen, the pooler, the idle token head
    assert [(s.begin, s.end) for s in segs] == [(e.off[i], e.off[i] + e.size[i]) for i in live]
    # adjacent tensors of one group with the same scalars (Q, K, V weights; their biases) stay apart
    q = IDX["encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.query.weight"]
    k = IDX["encoder.encoder.albert_layer_groups.0.albert_layers.0.attention.key.weight"]
    assert e.off[q] + e.size[q] == e.off[k] and group_of[q] == group_of[k] and q in live and k in live
    assert all(s.begin % 4 == 0 and s.end % 4 == 0 and s.begin < s.end and s.step == step for s in segs)
    assert all(a.end <= b.begin for a, b in zip(segs, segs[1:])) and max(s.end for s in segs) == e.train
    for s in segs:
        g = GROUPS[group_of[s.tensor]]
        assert (s.group, s.adapt) == (group_of[s.tensor], g["adapt"])
        want = R.scalars(g["lr"], g["betas"], g["eps"], g["weight_decay"], step)
        for key in R.SCALARS:
            assert _bits(getattr(s, key)) == _bits(want[key]), (NAMES[s.tensor], key)
    # one group for everything: still one segment per tensor; everything frozen: none
    assert len(e.plan(GROUPS[:1], [0] * _lib.PLB_NPARAM, 3)) == len([i for i, n in enumerate(NAMES) if e.size[i] and n not in POOLER + TOKEN])
    assert e.plan(GROUPS, [-1] * _lib.PLB_NPARAM, 3) == []
    floats = e.L.plb_lamb_floats(e.h)
    assert floats % 4 == 0 and floats >= 4 * _lib.PLB_NPARAM + 2 * sum((sz + 1023) // 1024 for sz, n in zip(e.size, NAMES) if n not in POOLER)


def test_refusals_have_a_text():
    e = Created(0)
    ok = [0] * _lib.PLB_NPARAM
    g = GROUPS[0]
    assert "n_groups" in e.plan([], ok, 1, expect=1)
    assert "group_of[0] = -2" in e.plan([g], [-2] + ok[1:], 1, expect=1)
    assert "adapt 2" in e.plan([{**g, "adapt": 2}], ok, 1, expect=1)
    assert "group 1: adapt -1" in e.plan([g, {**g, "adapt": -1}], ok, 1, expect=1)
    for key, bad in (("lr", -1e-3), ("lr", float("nan")), ("eps", -1e-8)):
        assert key in e.plan([{**g, key: bad}], ok, 1, expect=1)
    assert "beta1" in e.plan([{**g, "betas": (1.0, 0.999)}], ok, 1, expect=1)
    assert "beta2" in e.plan([{**g, "betas": (0.9, 1.0)}], ok, 1, expect=1)
    assert "step counts from 1" in e.plan([g], ok, 0, expect=1)
    L = e.L
    gof = (C.c_int32 * _lib.PLB_NPARAM)(*ok)
    assert L.plb_lamb_step(e.h, e.groups_c([g]), 1, gof, 1, 1.0, None, None, None) != 0
    assert b"not bound" in L.plb_last_error()
    inf = Created(0, inference_only=1)
    assert "inference-only" in inf.plan([g], ok, 1, expect=1)
    assert L.plb_lamb_step(inf.h, e.groups_c([g]), 1, gof, 1, 1.0, None, None, None) != 0


# ---- 3. Lamb.state_dict over a stand-in engine -----------------------------------------------------------------------------
def _cfg():
    return plbert_amd.AlbertConfig(vocab_size=188, embedding_size=64, hidden_size=128, num_attention_heads=2,
                                   intermediate_size=256, num_hidden_layers=2, max_position_embeddings=512)


class HostEngine:
    """What plbert_amd.train.AdamW / Lamb read of an engine outside ``step``: the layout and the flat moment buffers."""

    def __init__(self):
        shapes = plbert_amd.param_shapes(_cfg(), 188)
        self.layout, off = OrderedDict(), 0
        for n, shp in shapes.items():
            size = int(np.prod(shp))
            self.layout[n] = (off, size, tuple(shp))
            off += size
        self.total, self.num_tokens, self.token_head_steps = off, 0, 0
        self.trainable = self.layout[POOLER[0]][0]
        self.token_range = (off, off)
        self.exp_avg, self.exp_avg_sq = torch.zeros(off), torch.zeros(off)
        self._on_handoff_timeout = []

    def _bind(self):
        pass


class HostModel:
    def __init__(self):
        self.engine = HostEngine()
        self._params = [(n, torch.nn.Parameter(torch.zeros(shp))) for n, (_, _, shp) in self.engine.layout.items()]

    def named_parameters(self):
        return iter(self._params)


def test_lamb_state_dict_round_trips_and_loads_into_a_fresh_lamb():
    model = HostModel()
    named = list(model.named_parameters())
    nd = lambda n: "bias" in n or "LayerNorm" in n
    mk = lambda: [{"params": [p for n, p in named if "pooler" not in n and not nd(n)]},
                  {"params": [p for n, p in named if "pooler" not in n and nd(n)], "weight_decay": 0.0, "adapt": False, "lr": 5e-4}]
    opt = T.Lamb(mk(), lr=1e-3, model=model)
    assert isinstance(opt, T.AdamW) and opt.defaults["eps"] == 1e-6
    assert [g["adapt"] for g in opt.param_groups] == [None, False] and [g["lr"] for g in opt.param_groups] == [1e-3, 5e-4]
    # what three steps would leave: a step count, moments, and every grouped tensor stepped
    eng = model.engine
    eng.exp_avg.copy_(torch.randn(eng.total, generator=torch.Generator().manual_seed(1)))
    eng.exp_avg_sq.copy_(torch.rand(eng.total, generator=torch.Generator().manual_seed(2)))
    opt.step_count = 3
    opt._first_step = {n: 1 for n, _ in named if "pooler" not in n}
    sd = opt.state_dict()
    pool = [i for i, (n, _) in enumerate(named) if "pooler" in n]
    assert set(sd["state"]) == set(range(len(named))) - set(pool)
    assert all(float(st["step"]) == 3.0 and set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    assert [g["adapt"] for g in sd["param_groups"]] == [None, False] and sd["param_groups"][1]["weight_decay"] == 0.0
    assert "decoupled_weight_decay" not in sd["param_groups"][0] and sd["param_groups"][0]["betas"] == (0.9, 0.999)
    off, size, shp = eng.layout[named[0][0]]
    assert torch.equal(sd["state"][0]["exp_avg"], eng.exp_avg[off:off + size].view(shp))
    # ... into a fresh optimizer over a fresh model
    model2 = HostModel()
    named2 = list(model2.named_parameters())
    mk2 = lambda: [{"params": [p for n, p in named2 if "pooler" not in n and not nd(n)]},
                   {"params": [p for n, p in named2 if "pooler" not in n and nd(n)]}]
    opt2 = T.Lamb(mk2(), lr=9.0, model=model2)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 3 and [g["lr"] for g in opt2.param_groups] == [1e-3, 5e-4]
    assert [g["adapt"] for g in opt2.param_groups] == [None, False]
    n = eng.trainable
    assert torch.equal(model2.engine.exp_avg[:n], eng.exp_avg[:n]) and torch.equal(model2.engine.exp_avg_sq[:n], eng.exp_avg_sq[:n])
    again = opt2.state_dict()
    assert set(again["state"]) == set(sd["state"]) and again["param_groups"] == sd["param_groups"]
    for i in sd["state"]:
        assert torch.equal(again["state"][i]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
    with pytest.raises(ValueError, match="sizes"):
        T.Lamb([{"params": [p for _, p in named2]}], model=model2).load_state_dict(sd)
    # the layer adaptation: a group's own adapt wins, None decides by name; a plain parameter list is one group
    for p in (p for _, p in named):
        p.grad = torch.zeros_like(p)
    cut, cut_of = opt._live_groups()
    # (full_layer_layer_norm sits in the first group, whose adapt is None: the default exclusion names it)
    assert [(g["adapt"], g["weight_decay"]) for g in cut] == [(True, 0.01), (False, 0.01), (False, 0.0)]
    assert [n for n, k in cut_of.items() if k == 1] == [n for n, _ in named if n.endswith("full_layer_layer_norm.weight")]
    plain = T.Lamb([p for n, p in named if "pooler" not in n], model=model, exclude_from_layer_adaptation=("bias",))
    cut, cut_of = plain._live_groups()
    assert len(plain.param_groups) == 1 and [g["adapt"] for g in cut] == [True, False]
    assert all(cut[k]["adapt"] == ("bias" not in n) for n, k in cut_of.items()) and len(cut_of) == len(named) - 2


# ---- 4. the new symbols ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    for name in NEW_PUBLIC:
        assert name in _lib.PUBLIC and name in c_header.public().protos, name
    for name in NEW_INTERNAL:
        assert name in _lib.INTERNAL and name in c_header.kernels().protos, name
    assert "PlbLambGroup" in c_header.public().structs and "PlbLambSegment" in c_header.public().structs
    # the version script hides nothing of them ...
    script = open(os.path.join(c_header.ROOT, "plbert_amd", "csrc", "exports.map")).read()
    local = [pat.strip() for blk in re.findall(r"local:([^}]*)", re.sub(r"#[^\n]*", "", script)) for pat in blk.split(";") if pat.strip()]
    assert local and not [n for n in NEW_PUBLIC + NEW_INTERNAL for pat in local if fnmatch.fnmatch(n, pat)]
    # ... and the built library exports them
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-readelf")
    L = _lib.lib()
    out = subprocess.run([readelf, "--dyn-syms", "--wide", _lib.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = {ln.split()[7].split("@")[0] for ln in out.splitlines() if len(ln.split()) == 8 and ln.split()[6] != "UND"}
    for name in NEW_PUBLIC + NEW_INTERNAL:
        assert name in exported and getattr(L, name).argtypes == list({**_lib.PUBLIC, **_lib.INTERNAL}[name][1]), name
    assert "lamb.hip" in __import__("plbert_amd.build", fromlist=["SOURCES"]).SOURCES


# ---- 5. the default path ---------------------------------------------------------------------------------------------------
class RecordingEngine:
    """Stands in for HipEngine inside PLBertTrainer: the layout, and a record of the optimizer calls."""

    def __init__(self, cfg, num_phonemes, num_tokens=0, **kw):
        self.layout = HostEngine().layout
        self.device, self.num_tokens, self.calls, self._on_handoff_timeout = torch.device("cpu"), num_tokens, [], []
        self.packed_dual = self.packed_fp8 = False
        self.norm = torch.zeros(8)

    def load_state_dict(self, sd):
        pass

    def grad_norm(self, grad_scale=1.0, max_norm=0.0, have_partials=False, group_of=None):
        self.calls.append("plb_grad_norm" if group_of is None else "plb_grad_norm_groups")
        return self.norm

    def adamw_step(self, step, lr, betas, eps, weight_decay, grad_scale=1.0, norm_buf=None):
        self.calls.append("plb_adamw_step" if norm_buf is None else "plb_adamw_step_clipped")

    def adamw_plan(self, step, groups, group_of):
        return []

    def adamw_step_groups(self, step, groups, group_of, grad_scale=1.0, norm_buf=None):
        self.calls.append("plb_adamw_step_groups")

    def lamb_step(self, step, groups, group_of, grad_scale=1.0, norm_buf=None):
        self.calls.append("plb_lamb_step")
        self.last = (groups, group_of)


@pytest.mark.parametrize("kw,want", [
    ({}, ("plb_adamw_step",)),
    ({"max_grad_norm": 1.0}, ("plb_grad_norm", "plb_adamw_step_clipped")),
    ({"no_decay": ("bias",)}, ("plb_adamw_step_groups",)),
    ({"optimizer": "adamw", "frozen": ("position",), "max_grad_norm": 1.0}, ("plb_grad_norm_groups", "plb_adamw_step_groups")),
    ({"optimizer": "lamb"}, ("plb_lamb_step",)),
    ({"optimizer": "lamb", "max_grad_norm": 1.0, "no_decay": ("bias", "LayerNorm", "layer_norm")}, ("plb_grad_norm_groups", "plb_lamb_step")),
])
def test_a_trainer_without_optimizer_resolves_to_the_adamw_entry_points(monkeypatch, kw, want):
    monkeypatch.setattr(T, "HipEngine", RecordingEngine)
    tr = T.PLBertTrainer(_cfg(), 188, max_batch=2, max_seq=32, state_dict={}, **kw)
    assert tr.optimizer == kw.get("optimizer", "adamw")
    assert tr.optimizer_entry_points() == want                         # what it says it would call ...
    tr._optimizer_step(1.0)
    assert tuple(tr.engine.calls) == want and tr.step_count == 1       # ... is what the step calls
    if "optimizer" not in kw:
        assert not any("lamb" in c for c in tr.engine.calls)
        assert (tr.param_groups is None) == (not kw.get("no_decay"))
    if tr.optimizer == "lamb":
        groups, group_of = tr.engine.last
        assert all("adapt" in g for g in groups) and {g["adapt"] for g in groups} == {True, False}
        assert all(groups[k]["adapt"] == (not any(x in n for x in ("bias", "LayerNorm", "layer_norm"))) for n, k in group_of.items())
        assert set(group_of) == set(tr.engine.layout)
    with pytest.raises(ValueError, match="optimizer must be one of"):
        T.PLBertTrainer(_cfg(), 188, max_batch=2, max_seq=32, state_dict={}, optimizer="lars")


def test_the_driver_reads_the_optimizer_from_the_configuration(monkeypatch, tmp_path):
    from plbert_amd import run as RUN
    monkeypatch.setattr(T, "HipEngine", RecordingEngine)
    base = {"training_params": dict(batch_size=2, learning_rate=1e-3),
            "dataset_params": dict(max_seq_length=32),
            "model_params": dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, max_position_embeddings=512,
                                 num_hidden_layers=2, embedding_size=64, pretrained_model="")}
    tr, step = RUN.initialize_model(base, str(tmp_path), resuming=False)
    assert tr.optimizer == "adamw" and tr.param_groups is None and step == 0        # the key is absent: AdamW, one group
    assert tr.optimizer_entry_points() == ("plb_adamw_step",)
    lamb = {**base, "training_params": {**base["training_params"], "optimizer": "LAMB", "no_decay": ["bias"],
                                        "exclude_from_layer_adaptation": ["bias"]}}
    tr, _ = RUN.initialize_model(lamb, str(tmp_path), resuming=False)
    assert tr.optimizer == "lamb" and tr.optimizer_entry_points() == ("plb_lamb_step",)
    assert sorted((g["weight_decay"], g["adapt"]) for g in tr.param_groups) == [(0.0, False), (0.01, True)]
    assert all(("bias" in n) == (not g["adapt"]) for g in tr.param_groups for n in g["names"])
    with pytest.raises(ValueError, match="optimizer must be one of"):
        RUN.initialize_model({**base, "training_params": {**base["training_params"], "optimizer": "sgd"}}, str(tmp_path), False)
