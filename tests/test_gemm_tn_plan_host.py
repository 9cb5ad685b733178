"""plb_gemm_tn_plan (csrc/gemm_tn_plan.cpp) decides which kernel a token-major weight-gradient GEMM runs on, with how many
row splits, and how much slab that takes. Here, on the CPU, every field of the plan is compared with a restatement of the
rules as they stood BEFORE the plan unit existed: tn_big / tn_splits / weight_grad / weight_grad8 of engine_layers.cpp, the
argument lines of the three launchers, and the grids they launched. The restatement is written from that source as literals
and functions and imports nothing from the plan unit. The two environment knobs are read once per process, so each runs in a
child process. plb_create sizes the slabs from the plan: the workspace of every configuration below has the byte count it
had before. Last, the unit is compiled with a small main under AddressSanitizer + UBSan as a stand-alone program and swept
over zero, negative and near-2^31 arguments, holding each plan to its own consistency."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = list(_lib.TN_PLAN_FIELDS)
BF16, FP8 = 0, 1
SMALL, PIPELINE, PIPELINE_FP8 = 0, 1, 2
REFUSED = dict.fromkeys(FIELDS, 0)
REFUSED["rc"] = 1


# ---- the rules before the plan unit -------------------------------------------------------------------------------------
def tn_big(Mtot, Ncols, K):               # engine_layers.cpp
    return Ncols % 256 == 0 and K % 256 == 0 and Mtot >= 8192


def tn_splits(Mtot, N, K, fill_chip=True, cus=256):   # engine_layers.cpp; the knobs: PLBERT_TN_SPLITS=xcd, PLBERT_TN_CUS
    big = tn_big(Mtot, N, K)
    tiles = (N // 256) * (K // 256) if big else ((N + 127) // 128) * ((K + 127) // 128)
    splits = 768 // tiles
    if big:
        s = max(32 // tiles, 1)
        splits = 1 if tiles >= 256 else (max(cus // tiles, 1) if fill_chip else 8 * s)
    splits = max(min(splits, Mtot // 64), 1)
    rps = ((Mtot + splits - 1) // splits + 63) // 64 * 64
    return (Mtot + rps - 1) // rps, rps


def old_weight_grad(Mtot, Ncols, N, K, **knobs):       # weight_grad + plb_launch_gemm_tn / plb_launch_gemm_tn_big
    if Mtot <= 0 or N <= 0 or K <= 0 or N > Ncols:
        return dict(REFUSED)
    splits, rps = tn_splits(Mtot, N, K, **knobs)
    direct = splits == 1 and N == Ncols
    if N == Ncols and tn_big(Mtot, Ncols, K):
        if Ncols % 256 or K % 256 or rps % 64 or Mtot % 64 or splits * rps < Mtot:
            return dict(REFUSED)
        kernel, grid, block = PIPELINE, ((Ncols // 256) * (K // 256) * splits, 1), 512
    else:
        if Mtot % 64 or rps % 64 or K % 4 or splits * rps < Mtot:
            return dict(REFUSED)
        kernel, grid, block = SMALL, (((N + 127) // 128) * ((K + 127) // 128), splits), 256
    return dict(rc=0, kernel=kernel, splits=splits, rows_per_split=rps, direct=int(direct), grid_x=grid[0], grid_y=grid[1], block=block,
                slab_floats=0 if direct else splits * N * K, flops=2.0 * Mtot * N * K)


def old_weight_grad8(Mtot, Ncols, N, K, **knobs):      # weight_grad8 (Ncols = N there) + plb_launch_gemm_tn_fp8
    if Mtot <= 0 or N <= 0 or K <= 0 or N != Ncols:
        return dict(REFUSED)
    splits, rps = tn_splits(Mtot, N, K, **knobs)
    rps = (rps + 127) // 128 * 128
    splits = (Mtot + rps - 1) // rps
    if Ncols % 256 or K % 256 or rps % 128 or Mtot % 128 or splits * rps < Mtot:
        return dict(REFUSED)
    # (weight_grad8 always went through the slab; with one split the reduce copied what the kernel now stores itself)
    direct = splits == 1
    return dict(rc=0, kernel=PIPELINE_FP8, splits=splits, rows_per_split=rps, direct=int(direct), grid_x=(Ncols // 256) * (K // 256) * splits,
                grid_y=1, block=512, slab_floats=0 if direct else splits * N * K, flops=2.0 * Mtot * N * K)


def old_rules(Mtot, Ncols, N, K, ops, **knobs):
    return (old_weight_grad8 if ops == FP8 else old_weight_grad)(Mtot, Ncols, N, K, **knobs)


def old_tn8_ok(Mtot, H, I):               # engine_fp8.cpp
    return Mtot % 128 == 0 and H % 256 == 0 and I % 256 == 0 and Mtot >= 8192


def weights(H, I, E=128, NP=188, NTp=64000):           # (Ncols, N, K) of the seven weight gradients: engine.cpp's table
    return [(3 * H, 3 * H, H), (H, H, H), (I, I, H), (H, H, I), (H, H, E), (256, NP, H), (NTp, NTp, H)]


# 8128 / 8192 / 8256: the pipeline kernel's edge; 64 .. 1024: fewer 64-row K-tiles than splits; 192, 8256: multiples of 64, not of 128
MTOTS = [64, 128, 192, 320, 1024, 2048, 4096, 8128, 8192, 8256, 12288, 16384, 24576, 49152, 98304, 196608]
SHAPES = (weights(768, 2048) + weights(1024, 4096) +
          [(1024, 1024, 768),                                    # a token head of 1,000: 12 tiles
           (256, 4, 768), (256, 252, 768), (256, 256, 768),      # the phoneme head's range of NP
           (128, 128, 64), (384, 384, 128), (640, 636, 192), (2304, 2304, 772)])
assert len(SHAPES) == 22


def plan(L, Mtot, Ncols, N, K, ops):
    buf = C.create_string_buffer(struct.calcsize("8iqd"))   # PlbGemmTNPlan of csrc/gemm_tn_plan.h: eight ints, an int64, a double
    rc = L.plb_gemm_tn_plan(Mtot, Ncols, N, K, ops, buf)
    p = dict(zip(FIELDS, struct.unpack("8iqd", buf.raw)))
    assert rc == p["rc"]
    return p


def same(got, want, what):
    assert got == want, f"{what}: plan {got}, the engine's and the launchers' rules {want}"


def test_every_shape_and_operand_kind():
    L = _lib.lib()
    n = 0
    for Mtot, (Ncols, N, K), ops in itertools.product(MTOTS, SHAPES, (BF16, FP8)):
        same(plan(L, Mtot, Ncols, N, K, ops), old_rules(Mtot, Ncols, N, K, ops), (Mtot, Ncols, N, K, ops))
        n += 1
    assert n == 16 * 22 * 2
    assert _lib.gemm_tn_plan(196608, 2304, 2304, 768) == old_weight_grad(196608, 2304, 2304, 768)   # the dict form of the binding


def test_the_edges_the_rules_turn_on():
    L = _lib.lib()
    p = lambda *a: plan(L, *a)   # noqa: E731
    # the bench step's four layer weights: 9 / 28 / 10 / 10 splits, one workgroup per CU
    for (Ncols, N, K), splits in zip(weights(768, 2048)[:4], (9, 28, 10, 10)):
        q = p(196608, Ncols, N, K, BF16)
        assert (q["kernel"], q["splits"], q["direct"]) == (PIPELINE, splits, 0) and q["grid_x"] <= 256
    # below 8192 rows, or with a width that is no multiple of 256: the small kernel at 768 / tiles splits
    assert p(8128, 768, 768, 768, BF16)["kernel"] == SMALL and p(8192, 768, 768, 768, BF16)["kernel"] == PIPELINE
    assert p(16384, 768, 768, 128, BF16)["kernel"] == SMALL
    q = p(16384, 768, 768, 128, BF16)
    assert (q["splits"], q["grid_x"], q["grid_y"]) == (128, 6, 128)
    # fewer K-tiles than splits
    q = p(320, 768, 768, 768, BF16)
    assert (q["splits"], q["rows_per_split"]) == (5, 64)
    # the phoneme head: 256 readable columns, NP rows stored: never direct, never the pipeline kernel
    q = p(16384, 256, 188, 768, BF16)
    assert (q["kernel"], q["direct"], q["splits"], q["slab_floats"]) == (SMALL, 0, 64, 64 * 188 * 768)
    assert p(64, 256, 188, 768, BF16)["direct"] == 0 and p(64, 256, 188, 768, BF16)["splits"] == 1
    # the token head: 250 x 3 tiles need no row splits; the kernel writes the gradient itself
    q = p(16384, 64000, 64000, 768, BF16)
    assert (q["kernel"], q["splits"], q["direct"], q["slab_floats"], q["grid_x"]) == (PIPELINE, 1, 1, 0, 750)
    # fp8: 128-row K-tiles; the smallest call of the pipeline rule
    assert (p(8192, 256, 256, 256, BF16)["splits"], p(8192, 256, 256, 256, BF16)["rows_per_split"]) == (128, 64)
    assert (p(8192, 256, 256, 256, FP8)["splits"], p(8192, 256, 256, 256, FP8)["rows_per_split"]) == (64, 128)
    for Mtot in (192, 8256, 16448):
        assert Mtot % 64 == 0 and Mtot % 128 and p(Mtot, 768, 768, 768, FP8)["rc"] == 1 and p(Mtot, 768, 768, 768, BF16)["rc"] == 0
    assert p(16384, 768, 768, 128, FP8)["rc"] == 1 and p(16384, 256, 188, 768, FP8)["rc"] == 1
    # what does not exist
    for args in ((16384, 768, 768, 768, 2), (16384, 768, 768, 768, -1), (100, 768, 768, 768, BF16), (0, 768, 768, 768, BF16),
                 (16384, 768, 772, 768, BF16), (16384, 768, 768, 770, BF16), (16384, 768, 0, 768, BF16)):
        assert p(*args) == REFUSED, args


def test_the_engines_choice_of_the_fp8_images():
    """tn8_ok asks the plan: the bf16 plan of each layer weight is the pipeline kernel and the fp8 plan accepts the shape."""
    L = _lib.lib()
    for Mtot, (H, I) in itertools.product(MTOTS + [8064], ((768, 2048), (1024, 4096), (640, 2048), (768, 1920), (128, 512))):
        ok = all(plan(L, Mtot, n, n, k, BF16)["kernel"] == PIPELINE and plan(L, Mtot, n, n, k, BF16)["rc"] == 0 and
                 plan(L, Mtot, n, n, k, FP8)["rc"] == 0 for (_, n, k) in weights(H, I)[:4])
        assert ok == old_tn8_ok(Mtot, H, I), (Mtot, H, I)


CHILD = """
import json, sys
from plbert_amd import _lib
print(json.dumps([_lib.gemm_tn_plan(*a) for a in json.loads(sys.argv[1])]))
"""


@pytest.mark.parametrize("env, knobs", [({"PLBERT_TN_SPLITS": "xcd"}, dict(fill_chip=False)), ({"PLBERT_TN_CUS": "224"}, dict(cus=224)),
                                        ({"PLBERT_TN_CUS": "32"}, dict())], ids=["splits_xcd", "cus_224", "cus_out_of_range"])
def test_the_environment_knobs_in_a_fresh_process(env, knobs):
    args = [(Mtot, Ncols, N, K, ops) for Mtot in (4096, 8192, 16384, 196608) for (Ncols, N, K) in weights(768, 2048) + weights(1024, 4096)
            for ops in (BF16, FP8)]
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(args)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT,
                       env={**{k: v for k, v in os.environ.items() if not k.startswith("PLBERT_TN_")}, **env})
    assert r.returncode == 0, r.stdout[-3000:]
    got = json.loads(r.stdout.splitlines()[-1])
    changed = 0
    for a, g in zip(args, got):
        same(g, old_rules(*a, **knobs), (a, env))
        changed += g != old_rules(*a)
    assert (changed > 0) == bool(knobs)   # the knob was read (and an out-of-range value was not)


# plb_workspace_bytes at the commit before the plan unit: (hidden, heads, intermediate, layers, num_tokens, batch, seq, inference_only)
WORKSPACE_BYTES = {
    (768, 12, 2048, 12, 0, 32, 512, 0): 8962279936,
    (768, 12, 2048, 12, 0, 32, 512, 1): 513149440,
    (768, 12, 2048, 12, 64000, 32, 512, 0): 11711653888,
    (768, 12, 2048, 12, 64000, 32, 512, 1): 666183680,
    (768, 12, 2048, 12, 1000, 32, 512, 0): 9025377280,
    (1024, 16, 4096, 24, 0, 16, 512, 0): 14082566144,
    (1024, 16, 4096, 24, 0, 16, 512, 1): 423798784,
    (1024, 16, 4096, 24, 64000, 16, 512, 0): 15918982656,
    (1024, 16, 4096, 24, 64000, 16, 512, 1): 582428160,
    (768, 12, 2048, 12, 0, 2, 128, 0): 352059136,
    (768, 12, 2048, 12, 1000, 2, 128, 0): 359337472,
    (128, 2, 512, 2, 0, 4, 64, 0): 18019840,
}


def workspace_bytes(L, key):
    H, heads, I, layers, NT, B, S, inference = key
    c = _lib.PlbConfig(188, 128, H, heads, I, layers, 512, 2, 1e-12, 188, NT, B, S, inference)
    h = C.c_void_p()
    assert L.plb_create(C.byref(c), C.byref(h)) == 0, L.plb_last_error()
    ws = int(L.plb_workspace_bytes(h))
    L.plb_destroy(h)
    return ws


def test_the_workspace_is_sized_as_before():
    """plb_create and plb_workspace_bytes touch no device. The slab regions (o_slab, o_slab2) are sized from the plan; every
    other region is untouched, so an equal total means equal slabs."""
    L = _lib.lib()
    for key, want in WORKSPACE_BYTES.items():
        assert workspace_bytes(L, key) == want, key


SWEEP_MAIN = r"""
#include <cstdio>
#include "gemm_tn_plan.h"
int main() {
  const long long Ms[] = {-9223372036854775807LL - 1, -64, 0, 1, 64, 128, 192, 4096, 8128, 8192, 8256, 16384, 196608, 2147483520LL, 2147483584LL,
                          2147483647LL, 4294967296LL, 9223372036854775807LL};
  const int Ns[] = {-2147483647 - 1, -4, 0, 4, 124, 188, 256, 768, 1024, 2304, 64000, 2147483392, 2147483647};
  const int Ks[] = {-256, 0, 4, 6, 64, 128, 768, 2048, 2147483392, 2147483647};
  long runs = 0, sum = 0;
  for (long long M : Ms) for (int Ncols : Ns) for (int N : Ns) for (int K : Ks) for (int ops = -1; ops <= 2; ++ops) {
    PlbGemmTNPlan p;
    const int rc = plb_gemm_tn_plan(M, Ncols, N, K, ops, &p);
    bool ok = rc == p.rc;
    if (rc) ok = ok && !p.kernel && !p.splits && !p.rows_per_split && !p.direct && !p.grid_x && !p.grid_y && !p.block && !p.slab_floats && p.flops == 0;
    else ok = ok && p.splits >= 1 && p.rows_per_split % (ops == 1 ? 128 : 64) == 0 && (long long)p.splits * p.rows_per_split >= M &&
              (long long)(p.splits - 1) * p.rows_per_split < M && p.grid_x > 0 && p.grid_y > 0 && p.grid_y <= 65535 && p.block > 0 &&
              p.direct == (p.splits == 1 && N == Ncols) && p.slab_floats == (p.direct ? 0 : (long long)p.splits * N * K);
    if (!ok) {
      printf("inconsistent plan at %lld %d %d %d operands %d\n", M, Ncols, N, K, ops);
      return 1;
    }
    runs += rc == 0; sum += (long)p.grid_x + p.splits;
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
                        "-I", csrc, os.path.join(csrc, "gemm_tn_plan.cpp"), str(tmp_path / "main.cpp"), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0 and "plans that run" in r.stdout, r.stdout[-3000:]
