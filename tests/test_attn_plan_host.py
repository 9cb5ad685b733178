"""plb_attn_plan (csrc/attn_plan.cpp) decides what the attention launchers run: grid and kernel variant, the form of the
backward under the policy in force, the partial rows of the Q/K/V bias gradient, the float count of the statistics, the
profiler's credit, and whether a packed slot has rows no attention launch writes. Here, on the CPU, every field of the plan is
compared with a restatement of the rules as they stood BEFORE the plan unit existed: check_attn / plb_launch_attn_fwd /
launch_attn_bwd_split / attn_samples / plb_launch_attn_bwd of attn.hip, plb_launch_attn_bwd_fused of attn_bwd_fused.hip,
plb_launch_attn_probs_masked of layer_outputs.hip, qkvcol_rows and the `row_start && S % 128` guards of engine_layers.cpp and
the capacity of engine.cpp. The restatement is written from that source as literals and functions and imports nothing from the
plan unit. PLBERT_ATTN_BWD is read once per process, so each value runs in a child process. The launchers' one argument check
runs before any HIP call, so its refusals are exercised here too, on descriptors whose pointers are never followed.
plb_create sizes the partial rows from the plan: the workspace of every configuration of the weight-gradient plan's test
keeps its byte count. Last, the unit is compiled with a small main under AddressSanitizer + UBSan as a stand-alone program
and swept over zero, negative and near-2^31 arguments, holding each plan to its own consistency."""
import ctypes as C
import itertools
import json
import os
import shutil
import struct
import subprocess
import sys

import pytest

from plbert_amd import _lib
from test_gemm_tn_plan_host import WORKSPACE_BYTES, workspace_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("rc", "grid", "block", "km", "bwd_form", "bwd_one_samples", "bwd_one_grid", "colpart_rows", "colpart_sample_rows",
          "unwritten_rows", "cls_fwd", "cls_bwd_dq", "cls_bwd_dkv", "cls_bwd_one", "stat_floats", "fwd_flops", "fwd_bytes",
          "bwd_flops", "bwd_bytes")
FORMAT = "14iq4d"   # PlbAttnPlan of csrc/attn_plan.h: fourteen ints, an int64, four doubles
PACKED, KEYMASK, COMPACT, ROWS, IMAGE = 1, 2, 4, 8, 16
TWO, ONE, HYBRID = 0, 1, 2
REFUSED = dict.fromkeys(FIELDS, 0)
REFUSED["rc"] = 1
# engine_prof.cpp's class table at the parent commit: the classes the four launch sites passed to plb_prof_begin
CLS = {"attn_fwd": 5, "attn_bwd_dq": 6, "attn_bwd_dkv": 7, "attn_bwd": 22}


# ---- the rules before the plan unit -------------------------------------------------------------------------------------
def old_policy(value):                       # plb_set_attn_bwd_fused
    return -1 if value < 0 else (1 if value > 2 else value)


def old_env_policy(text):                    # plb_launch_attn_bwd, first launch
    return {"fused": 1, "split": 0, "hybrid": 2}.get(text, -1)


def old_fused_samples(B, S, NH, flags, policy):   # plb_launch_attn_bwd: the samples plb_launch_attn_bwd_fused got
    can_fuse = S <= 512 and not (flags & ROWS and flags & IMAGE) and not flags & COMPACT and not flags & KEYMASK
    if not can_fuse or policy == 0:
        return 0
    if policy == 1:
        return B
    if S <= 384:
        return 0
    items = B * NH
    rounds = (items + 255) // 256
    if items * 10 >= rounds * 256 * 9:
        return B
    per_round = 256 // NH
    full = B // per_round if per_round > 0 else 0
    nb_f, rest = full * per_round, B - full * per_round
    if policy == 2 and full >= 1 and per_round * NH * 10 >= 256 * 9 and rest * NH <= 160:
        return nb_f
    return 0


def old_rules(B, S, NH, flags, policy):
    if B < 1 or S < 1 or NH < 1:                                       # check_attn (H = NH * 64 has no NH < 1)
        return dict(REFUSED)
    if flags & KEYMASK and (S > 2048 or flags & COMPACT):             # check_attn
        return dict(REFUSED)
    qt = (S + 127) // 128
    grid = qt * NH * B                                                  # the three launchers
    if grid >= 1 << 31 or B * qt * 4 >= 1 << 31:                        # plb_launch_attn_probs_masked; what an int holds
        return dict(REFUSED)
    nf = old_fused_samples(B, S, NH, flags, policy)
    unit = float(B) * NH * float(S) * S * 64.0
    io = 2.0 * B * S * float(NH * 64)
    return dict(rc=0, grid=grid, block=256, km=int(bool(flags & KEYMASK)), bwd_form=TWO if nf == 0 else ONE if nf == B else HYBRID,
                bwd_one_samples=nf, bwd_one_grid=NH * nf,               # plb_launch_attn_bwd_fused: grid(NH * B) of its call
                colpart_rows=B * qt * 4, colpart_sample_rows=qt * 4,   # qkvcol_rows; attn_samples: b0 * ceil(S/128) * 4 rows
                unwritten_rows=int(bool(flags & PACKED) and S % 128 != 0),   # engine_layers.cpp: rw.row_start && S % 128
                cls_fwd=CLS["attn_fwd"], cls_bwd_dq=CLS["attn_bwd_dq"], cls_bwd_dkv=CLS["attn_bwd_dkv"], cls_bwd_one=CLS["attn_bwd"],
                stat_floats=B * NH * S,                                 # engine.cpp / slots(): lse and delta
                fwd_flops=4.0 * unit, fwd_bytes=4.0 * io,               # plb_launch_attn_fwd
                bwd_flops=8.0 * unit, bwd_bytes=6.0 * io)               # fused: 8 unit, 6 io; split: 4 unit and 6 io per kernel


BS = range(1, 41)
NHS = (1, 2, 4, 12, 16)
SS = (1, 64, 127, 128, 129, 200, 384, 385, 448, 512, 513, 2048, 2049)


def plan(L, buf, B, S, NH, flags):
    rc = L.plb_attn_plan(B, S, NH, flags, buf)
    p = dict(zip(FIELDS, struct.unpack(FORMAT, buf.raw)))
    assert rc == p["rc"]
    return p


def test_the_binding_names_the_structs_fields():
    assert FIELDS == _lib.ATTN_PLAN_FIELDS and FORMAT == _lib.ATTN_PLAN_FORMAT
    assert (PACKED, KEYMASK, COMPACT, ROWS, IMAGE) == (_lib.ATTN_PACKED, _lib.ATTN_KEYMASK, _lib.ATTN_COMPACT, _lib.ATTN_OUT_ROWS,
                                                       _lib.ATTN_OUT_IMAGE)
    L = _lib.lib()
    names = [L.plb_profile_class_name(i).decode() for i in range(L.plb_profile_num_classes())]
    assert {n: names.index(n) for n in CLS} == CLS


@pytest.mark.parametrize("policy", [-1, 0, 1, 2])
def test_every_shape_flag_set_and_policy(policy):
    L = _lib.lib()
    buf = C.create_string_buffer(struct.calcsize(FORMAT))
    L.plb_set_attn_bwd_fused(policy)
    try:
        n = forms = 0
        for B, NH, S, flags in itertools.product(BS, NHS, SS, range(32)):
            got, want = plan(L, buf, B, S, NH, flags), old_rules(B, S, NH, flags, policy)
            assert got == want, f"{(B, S, NH, flags, policy)}: plan {got}, the launchers' and the engine's rules {want}"
            n += 1
            forms |= 1 << got["bwd_form"] if got["rc"] == 0 else 0
        assert n == 40 * 5 * 13 * 32
        assert forms == {-1: 0b011, 0: 0b001, 1: 0b011, 2: 0b111}[policy]   # the sweep reaches every form the policy has
        assert _lib.attn_plan(32, 512, 12, ROWS) == old_rules(32, 512, 12, ROWS, policy)   # the dict form of the binding
    finally:
        L.plb_set_attn_bwd_fused(-1)


def test_the_setters_value_mapping_and_the_edges_the_policy_turns_on():
    L = _lib.lib()
    buf = C.create_string_buffer(struct.calcsize(FORMAT))
    try:
        for value in (-7, -1, 0, 1, 2, 3, 9):
            L.plb_set_attn_bwd_fused(value)
            for B, S, NH in ((16, 512, 16), (32, 512, 12), (22, 512, 12), (8, 512, 12), (4, 384, 4)):
                assert plan(L, buf, B, S, NH, ROWS) == old_rules(B, S, NH, ROWS, old_policy(value)), (value, B, S, NH)
        p = lambda pol, *a: (L.plb_set_attn_bwd_fused(pol), plan(L, buf, *a))[1]   # noqa: E731
        # auto: 16 x 16 = one full round -> the single kernel; 32 x 12 = 1.5 rounds, 8 x 12 = 96 items -> two kernels
        assert [p(-1, B, 512, NH, ROWS)["bwd_one_samples"] for B, NH in ((16, 16), (32, 12), (8, 12))] == [16, 0, 0]
        # the 384 / 512 bounds
        assert [p(-1, 16, S, 16, ROWS)["bwd_form"] for S in (384, 385, 512, 513)] == [TWO, ONE, ONE, TWO]
        assert [p(1, 3, S, 2, ROWS)["bwd_form"] for S in (1, 384, 512, 513)] == [ONE, ONE, ONE, TWO]
        # the last round at least 90 % full of 256: 231 items (one round, 90.2 %) yes, 230 no; 487 of 512 (95 %) yes
        assert [p(-1, B, 512, 1, ROWS)["bwd_form"] for B in (230, 231, 256, 257, 460, 461)] == [TWO, ONE, ONE, TWO, TWO, ONE]
        # hybrid: 21 samples of 12 heads = 252 items per round; a remainder of at most 160 items
        assert [p(2, B, 512, 12, ROWS)["bwd_one_samples"] for B in (8, 21, 22, 32, 34, 35, 42, 43)] == [0, 21, 21, 21, 21, 0, 42, 42]
        assert p(2, 34, 512, 12, ROWS)["bwd_form"] == HYBRID and p(2, 34, 512, 12, ROWS)["bwd_one_grid"] == 252
        # key masks, compact queries and rows + image: the two kernels, whatever the policy
        for pol, flags in itertools.product((-1, 1, 2), (KEYMASK, COMPACT, ROWS | IMAGE, PACKED | KEYMASK | IMAGE)):
            assert p(pol, 16, 512, 16, flags)["bwd_form"] == TWO, (pol, flags)
        assert p(1, 16, 512, 16, IMAGE)["bwd_form"] == ONE and p(1, 16, 512, 16, PACKED | ROWS)["bwd_form"] == ONE
        # what does not exist
        for args in ((0, 512, 12, 0), (4, 0, 12, 0), (4, 512, 0, 0), (-1, 512, 12, 0), (4, 2049, 2, KEYMASK), (4, 512, 2, KEYMASK | COMPACT),
                     (1 << 26, 1, 32, 0), (1 << 24, 129, 64, 0), (1 << 29, 1, 1, 0)):
            assert p(-1, *args) == REFUSED, args
        assert p(-1, (1 << 26) - 1, 1, 32, 0)["grid"] == (1 << 31) - 32 and p(-1, (1 << 29) - 1, 1, 1, 0)["colpart_rows"] == (1 << 31) - 4
    finally:
        L.plb_set_attn_bwd_fused(-1)


CHILD = """
import json, sys
from plbert_amd import _lib
args = json.loads(sys.argv[1])
first = [_lib.attn_plan(*a) for a in args]
_lib.lib().plb_set_attn_bwd_fused(0)
print(json.dumps([first, [_lib.attn_plan(*a) for a in args]]))
"""


@pytest.mark.parametrize("value", ["fused", "split", "auto", "hybrid"])
def test_the_environment_policy_in_a_fresh_process(value):
    args = [(B, S, NH, flags) for B in (8, 16, 22, 32) for S in (384, 448, 512, 513) for NH in (12, 16) for flags in (ROWS, IMAGE, ROWS | IMAGE)]
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(args)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT,
                       env={**os.environ, "PLBERT_ATTN_BWD": value})
    assert r.returncode == 0, r.stdout[-3000:]
    first, after_setter = json.loads(r.stdout.splitlines()[-1])
    for a, g, h in zip(args, first, after_setter):
        assert g == old_rules(*a, old_env_policy(value)), (a, value)
        assert h == old_rules(*a, 0), (a, value)      # a setter call overrides the environment
    forms = {g["bwd_form"] for g in first}
    assert forms == {"fused": {ONE, TWO}, "split": {TWO}, "auto": {ONE, TWO}, "hybrid": {ONE, TWO, HYBRID}}[value]


# ---- the launchers' one argument check -----------------------------------------------------------------------------------
FWD, BWD, BWD_SINGLE, PROBS = 0, 1, 2, 3
PTR = 0x10000   # a pointer no refused call follows: the check runs before any HIP call


def descriptor(B=2, S=512, NH=2, **over):
    H = NH * 64
    p = _lib.PlbAttn()
    p.qkv, p.ldqkv, p.B, p.S, p.NH, p.H, p.scale = PTR, 3 * H, B, S, NH, H, 0.125
    p.ctx, p.ldctx, p.lse = PTR, H, PTR
    p.dctx, p.lddctx, p.delta, p.dqkv, p.lddqkv = PTR, H, PTR, PTR, 3 * H
    for k, v in over.items():
        setattr(p, k, v)
    return p


def keymask(keys, **over):
    return {"key_words": PTR, "ldkw": 2 * ((keys + 63) // 64), **over}


COMPACT_Q = dict(qoff=PTR, q=PTR, ldq=128, nq_total=40, dq=PTR, lddq=128)
IMAGE8 = dict(dqkv8=PTR, lddqkv8=384, dqkv_scale=PTR)
# bad descriptors of every direction; then those of the forward and the backward launchers; then each launcher's own
BAD_ANY = {
    "null qkv": dict(qkv=None), "null lse": dict(lse=None), "ldqkv % 8": dict(ldqkv=388), "H is not NH * 64": dict(H=192),
    "no sample": dict(B=0), "no position": dict(S=0), "no head": dict(NH=0, H=0),
    "packed without lengths": dict(row_start=PTR), "ldkw too small": keymask(512, ldkw=15),
    "S > 2048 with words": keymask(2049, S=2049), "key mask with compact queries": {**keymask(512), **COMPACT_Q},
    "a grid of 2^31": dict(B=1 << 26, S=1, NH=32, H=2048, ldqkv=6144),
    "32-bit staging offsets": dict(S=2048, ldqkv=1 << 20),
}
BAD_FWD_BWD = {"null ctx": dict(ctx=None), "ldctx % 8": dict(ldctx=132), "compact queries without q": {**COMPACT_Q, "q": None},
               "ldq % 8": {**COMPACT_Q, "ldq": 132}, "negative nq_total": {**COMPACT_Q, "nq_total": -1}}
BAD_FWD = {"image without its scale": dict(ctx8=PTR, ldctx8=128), "ldctx8 % 8": dict(ctx8=PTR, ldctx8=132, ctx_scale=PTR)}
BAD_BWD = {"null dctx": dict(dctx=None), "lddctx % 8": dict(lddctx=132), "lddqkv % 8": dict(lddqkv=388), "no output": dict(dqkv=None),
           "image without its scale": {**IMAGE8, "dqkv_scale": None}, "lddqkv8 % 8": {**IMAGE8, "lddqkv8": 388},
           "compact queries without dq": {**COMPACT_Q, "dq": None}, "lddq % 8": {**COMPACT_Q, "lddq": 132},
           "lddq8 % 8": {**COMPACT_Q, "dq8": PTR, "lddq8": 132}}
BAD_SINGLE = {"S > 512": dict(S=513), "key mask": keymask(512), "compact queries": COMPACT_Q, "rows and image": IMAGE8}
GOOD = {FWD: [dict(), keymask(512), COMPACT_Q, dict(ctx8=PTR, ldctx8=128, ctx_scale=PTR), dict(row_start=PTR, lengths=PTR), dict(S=2048, ldqkv=(1 << 20) - 8)],
        BWD: [dict(), keymask(512), COMPACT_Q, IMAGE8, {**IMAGE8, "dqkv": None}, dict(S=513), dict(delta=None)],
        BWD_SINGLE: [dict(), {**IMAGE8, "dqkv": None}, dict(row_start=PTR, lengths=PTR), dict(S=1)],
        PROBS: [dict(ctx=None, dctx=None, dqkv=None), keymask(512, ctx=None), dict(S=2049)]}


def test_the_argument_check_by_direction():
    L = _lib.lib()
    bad = {FWD: {**BAD_ANY, **BAD_FWD_BWD, **BAD_FWD}, BWD: {**BAD_ANY, **BAD_FWD_BWD, **BAD_BWD},
           BWD_SINGLE: {**BAD_ANY, **BAD_FWD_BWD, **BAD_BWD, **BAD_SINGLE}, PROBS: BAD_ANY}
    for direction in (FWD, BWD, BWD_SINGLE, PROBS):
        for over in GOOD[direction]:
            assert L.plb_attn_args_check(C.byref(descriptor(**over)), direction) == 0, (direction, over)
        for why, over in bad[direction].items():
            assert L.plb_attn_args_check(C.byref(descriptor(**over)), direction) == 1, (direction, why)
    assert L.plb_attn_args_check(None, FWD) == 1 and L.plb_attn_args_check(C.byref(descriptor()), 4) == 1
    # what only one direction refuses is accepted by the others
    for why, over in BAD_SINGLE.items():
        assert L.plb_attn_args_check(C.byref(descriptor(**over)), BWD) == 0, why
    assert L.plb_attn_args_check(C.byref(descriptor(dctx=None, dqkv=None)), FWD) == 0


def test_every_launcher_refuses_before_any_hip_call():
    """1 is the launchers' refusal; a descriptor that got past the check would reach the launch and, without a device,
    come back as 2."""
    L = _lib.lib()
    launchers = {"plb_launch_attn_fwd": {**BAD_ANY, **BAD_FWD_BWD, **BAD_FWD}, "plb_launch_attn_bwd": {**BAD_ANY, **BAD_FWD_BWD, **BAD_BWD},
                 "plb_launch_attn_bwd_fused": {**BAD_ANY, **BAD_FWD_BWD, **BAD_BWD, **BAD_SINGLE}}
    for name, cases in launchers.items():
        for why, over in cases.items():
            assert getattr(L, name)(C.byref(descriptor(**over)), None) == 1, (name, why)

    def probs(qkv=PTR, ldqkv=384, lse=PTR, lengths=None, row_start=None, key_words=None, ldkw=0, B=2, S=512, NH=2, out=PTR):
        return L.plb_launch_attn_probs_masked(qkv, ldqkv, lse, lengths, row_start, key_words, ldkw, B, S, NH, 0.125, out, None)

    for why, over in {"null qkv": dict(qkv=None), "null lse": dict(lse=None), "null out": dict(out=None), "ldqkv % 8": dict(ldqkv=388),
                      "ldqkv below 3H": dict(ldqkv=376), "qkv off 16 bytes": dict(qkv=PTR + 8), "out off 4 bytes": dict(out=PTR + 2),
                      "no sample": dict(B=0), "no position": dict(S=0), "no head": dict(NH=0), "packed without lengths": dict(row_start=PTR),
                      "ldkw too small": dict(key_words=PTR, ldkw=15), "S > 2048 with words": dict(key_words=PTR, ldkw=66, S=2049),
                      "a grid of 2^31": dict(B=1 << 26, S=1, NH=32, ldqkv=6144), "32-bit staging offsets": dict(S=2048, ldqkv=1 << 20)}.items():
        assert probs(**over) == 1, why
    assert L.plb_launch_attn_probs(None, 384, PTR, None, None, 2, 512, 2, 0.125, PTR, None) == 1


def test_the_workspace_is_sized_as_before():
    """The Q/K/V bias partial rows of plb_create are the plan's at (max_batch, max_seq); every other region is untouched."""
    L = _lib.lib()
    for key, want in WORKSPACE_BYTES.items():
        assert workspace_bytes(L, key) == want, key


SWEEP_MAIN = r"""
#include <cstdio>
#include <cstring>
#include "attn_plan.h"
extern "C" void plb_set_attn_bwd_fused(int on);
int main() {
  const int Bs[] = {-2147483647 - 1, -1, 0, 1, 2, 16, 21, 22, 32, 255, 256, 257, 65536, 1 << 24, 1 << 26, (1 << 29) - 1, 1 << 29, 2147483647};
  const int Ss[] = {-2147483647 - 1, -128, 0, 1, 127, 128, 129, 384, 385, 512, 513, 2048, 2049, 65536, 2147483519, 2147483520, 2147483647};
  const int NHs[] = {-2147483647 - 1, -1, 0, 1, 2, 12, 16, 32, 255, 256, 257, 1 << 24, 2147483647};
  const PlbAttnPlan zero = {};
  long runs = 0, sum = 0;
  for (int pol = -2; pol <= 3; ++pol) {
    plb_set_attn_bwd_fused(pol);
    for (int B : Bs) for (int S : Ss) for (int NH : NHs) for (int flags = -1; flags <= 32; ++flags) {
      PlbAttnPlan p;
      memset(&p, 0x5a, sizeof(p));
      const int rc = plb_attn_plan(B, S, NH, flags, &p);
      bool ok = rc == p.rc;
      if (rc) {
        PlbAttnPlan q = p;
        q.rc = 0;
        ok = ok && rc == 1 && !memcmp(&q, &zero, sizeof(q));
      } else {
        const long long qt = ((long long)S + 127) / 128;
        ok = ok && B >= 1 && S >= 1 && NH >= 1 && p.grid == qt * NH * B && p.block == 256 && p.colpart_rows == qt * 4 * B &&
             p.colpart_sample_rows * (long long)B == p.colpart_rows && p.km == ((flags & PLB_ATTN_KEYMASK) != 0) &&
             p.bwd_one_samples >= 0 && p.bwd_one_samples <= B && p.bwd_one_grid == (long long)NH * p.bwd_one_samples &&
             p.bwd_form == (p.bwd_one_samples == 0 ? PLB_ATTN_BWD_TWO : p.bwd_one_samples == B ? PLB_ATTN_BWD_ONE : PLB_ATTN_BWD_HYBRID) &&
             (p.bwd_one_samples == 0 || (S <= 512 && !(flags & (PLB_ATTN_KEYMASK | PLB_ATTN_COMPACT)))) &&
             p.stat_floats == (long long)B * NH * S && p.unwritten_rows == ((flags & PLB_ATTN_PACKED) && S % 128 != 0) &&
             p.fwd_flops > 0 && p.bwd_flops == 2 * p.fwd_flops && p.fwd_bytes > 0 && p.bwd_bytes == 1.5 * p.fwd_bytes;
      }
      if (!ok) {
        printf("inconsistent plan at B %d S %d NH %d flags %d policy %d\n", B, S, NH, flags, pol);
        return 1;
      }
      runs += rc == 0; sum += (long)p.grid + p.bwd_one_samples;
    }
  }
  printf("plans that run: %ld, checksum %ld\n", runs, sum);
  return 0;
}
"""


def test_the_plan_unit_under_address_and_ub_sanitizers(tmp_path):
    """The unit is plain C++ with no HIP header: compiled with the host compiler and a main of its own, instrumented, and
    run as a program."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "plbert_amd", "csrc")
    (tmp_path / "main.cpp").write_text(SWEEP_MAIN)
    exe = tmp_path / "plan_sweep"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", csrc, os.path.join(csrc, "attn_plan.cpp"), str(tmp_path / "main.cpp"), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0 and "plans that run" in r.stdout, r.stdout[-3000:]
