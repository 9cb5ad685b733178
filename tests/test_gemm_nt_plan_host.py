"""plb_gemm_nt_plan (csrc/gemm_nt_plan.cpp) decides what every NT GEMM launcher does. Here, on the CPU, every field of the plan
is compared with a restatement of the rules as they stood BEFORE the plan unit existed, when each launcher and the engine
carried their own copy: pick_tile / small_tile / plb_gemm_nt_colpart_rows of gemm.hip, launch_big and the K-loop choice of
gemm_big.hip, the tile rules of gemm_fp8.hip, gemm_ln.hip and gemm_fp8_ln.hip, the shape half of ln_launch_check, the token
head's tile line of engine_calls.cpp, the five byte formulas and the class choices. The restatement below is written from
that source as literals and functions; it imports nothing from the plan unit. A second check compiles the unit with a small
main under AddressSanitizer + UBSan as a stand-alone program: a memory / undefined-behaviour check over a wider grid (zero,
negative and near-2^31 shapes, unknown forms) that holds each plan to its own consistency only, not to the rules above."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

from plbert_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Plan(C.Structure):   # PlbGemmNTPlan of csrc/gemm_nt_plan.h
    _fields_ = [(n, C.c_int32) for n in ("rc", "family", "tile", "tile_m", "tile_n", "kloop", "grid", "block", "cls", "colpart_rows")] + \
               [("flops", C.c_double), ("bytes", C.c_double)]


FIELDS = [n for n, _ in Plan._fields_]
PLAIN, GELU, GELUBWD, CE1, CE2, LNFWD, LNBWD, GELUD, GELUDBWD, F32 = range(10)
BF16, E4M3, E5M2 = range(3)
COLPART, RES, C8, OUT16 = 1, 2, 4, 8
# PlbKernelClass, by position in engine_prof.cpp's name table
K_NT, K_GELU, K_GELUBWD, K_F32 = 0, 1, 2, 3
K_CE, K_SMALL = 19, 20
K_FP8, K_GELU_FP8, K_GELUBWD_FP8, K_LNFWD, K_LNBWD, K_LNFWD_FP8, K_LNBWD_FP8 = 23, 24, 25, 26, 27, 28, 29

MS = [64, 128, 192, 256, 384, 512, 1024, 1920, 2048, 2304, 3072, 8192, 16384, 49152]
NS = [4, 124, 128, 188, 256, 384, 512, 768, 1024, 1536, 2048, 2304, 3072, 4096, 5120, 64000]   # 64000 = 250 x 256
KS = [64, 128, 192, 768, 2048]
# beside the grid: 5 column tiles of the LayerNorm forms (1280 = 5 x 256, 1920 = 5 x 384) and the 64x64 rule's edge
EXTRA = [(1024, 1280, 128), (1024, 1920, 128), (2048, 1280, 768), (32640, 124, 64), (32768, 124, 64), (1920, 2176, 64)]


def plan(L, M, N, K, form, ops, opts, tile=0):
    p = Plan()
    rc = L.plb_gemm_nt_plan(M, N, K, form, ops, opts, tile, C.byref(p))
    assert rc == p.rc
    return {n: getattr(p, n) for n in FIELDS}


# ---- the rules before the plan unit -------------------------------------------------------------------------------------
def pick_tile(M, N, g_tile):          # gemm.hip
    ok256 = M % 256 == 0 and N % 256 == 0
    ok384 = M % 128 == 0 and N % 384 == 0
    ok1256 = M % 128 == 0 and N % 256 == 0
    if g_tile == 128:
        return 128
    if g_tile == 256:
        return 256 if ok256 else 128
    if g_tile == 384:
        return 384 if ok384 else (256 if ok256 else 128)
    if g_tile == 1256:
        return 1256 if ok1256 else 128
    if M * N < 256 * 256 * 64:
        return 128

    def eff(ok, tm, tn, handicap):
        if not ok:
            return 0.0
        t = (M // tm) * (N // tn)
        return handicap * t / (((t + 255) // 256) * 256)
    e256, e384, e1256 = eff(ok256, 256, 256, 1.0), eff(ok384, 128, 384, 0.95), eff(ok1256, 128, 256, 0.85)
    if e256 == 0 and e384 == 0 and e1256 == 0:
        return 128
    if e1256 > e256 and e1256 > e384:
        return 1256
    return 384 if e384 > e256 else 256


def small_tile(M, N, g_tile, env=0):   # gemm.hip (env: PLBERT_NT_SMALL_TILE, unset in the suite)
    if g_tile == 64:
        return 64
    if g_tile in (-64, 128):
        return 128
    if env:
        return env
    return 64 if (M // 128) * ((N + 127) // 128) < 256 else 128


DIMS = {256: (256, 256), 384: (128, 384), 1256: (128, 256)}
REFUSED = dict.fromkeys(FIELDS, 0)


def refused(rc):
    return dict(REFUSED, rc=rc)


def pipeline(M, N, K, tile, kloop, cls, nbytes, colpart_rows):
    tm, tn = DIMS[tile]
    return dict(rc=0, family=1, tile=tile, tile_m=tm, tile_n=tn, kloop=kloop, grid=(M // tm) * (N // tn), block=512, cls=cls,
                colpart_rows=colpart_rows, flops=2.0 * M * N * K, bytes=float(nbytes))


def act_of(form):
    return 0 if form == F32 else form


def prefetch(tile, act, g_pf):         # plb_launch_gemm_nt_big
    return int(tile != 256 or act != 0) if g_pf < 0 else int(g_pf != 0)


def bytes_nt(M, N, K, form, opts):     # plb_launch_gemm_nt
    act = act_of(form)
    return 2.0 * (M * K + N * K) + M * N * (4 if form == F32 else 4 if act == 1 else 2) + (2.0 * M * N if opts & RES else 0.0) + \
        (2.0 * M * N if act == 2 else 0.0)


def old_launch_gemm_nt(M, N, K, form, opts, g_tile, g_pf):
    if M % 128 or K % 64 or N % 4 or M <= 0 or N <= 0 or K <= 0:
        return refused(1)
    cls = K_F32 if form == F32 else {0: K_NT, 1: K_GELU, 2: K_GELUBWD}[form]
    tile = pick_tile(M, N, g_tile)
    if opts & COLPART and tile == 128:
        return refused(1)
    if tile != 128:   # launch_big's shape lines hold for every tile pick_tile returns
        tm = DIMS[tile][0]
        return pipeline(M, N, K, tile, prefetch(tile, act_of(form), g_pf), cls, bytes_nt(M, N, K, form, opts),
                        2 * (M // tm) if opts & COLPART else 0)
    st = small_tile(M, N, g_tile)
    return dict(rc=0, family=0, tile=st, tile_m=st, tile_n=st, kloop=-1, grid=(M // st) * ((N + st - 1) // st), block=256,
                cls=K_F32 if form == F32 else K_SMALL, colpart_rows=0, flops=2.0 * M * N * K, bytes=bytes_nt(M, N, K, form, opts))


def old_launch_big(M, N, K, tile, form, opts, g_pf):   # gemm_big.hip with the caller's tile; the token head's class for 3 / 4
    tm, tn = DIMS[tile]
    if M % tm or N % tn or K % 64 or M <= 0 or N <= 0 or K <= 0:
        return refused(1)
    if form in (CE1, CE2):
        if tn != 256:
            return refused(1)
        return pipeline(M, N, K, tile, prefetch(tile, form, g_pf), K_CE, 0.0, 2 * (M // tm) if opts & COLPART else 0)
    cls = K_F32 if form == F32 else {0: K_NT, 1: K_GELU, 2: K_GELUBWD}[form]
    return pipeline(M, N, K, tile, prefetch(tile, act_of(form), g_pf), cls, bytes_nt(M, N, K, form, opts),
                    2 * (M // tm) if opts & COLPART else 0)


def old_token_head(M, N, K, form, opts, g_pf):          # engine_calls.cpp: token_head's tile line + plb_launch_gemm_nt_big
    return old_launch_big(M, N, K, 256 if M % 256 == 0 else 1256, form, opts, g_pf)


def old_fp8(M, N, K, form, opts):                       # gemm_fp8.hip
    if M % 128 or K % 128:
        return refused(3)
    if form == PLAIN and N % 384 == 0:
        tile = 384
    elif N % 256 == 0:
        tile = 1256
    else:
        return refused(3)
    if M <= 0 or N <= 0 or K <= 0:
        return refused(3)
    nbytes = (M * K + N * K) + M * N * (4 if form == GELU else 2) + (2.0 * M * N if opts & RES else 0.0) + \
        (2.0 * M * N if form == GELUBWD else 0.0) + (M * N if opts & C8 else 0.0)
    return pipeline(M, N, K, tile, 1, {0: K_FP8, 1: K_GELU_FP8, 2: K_GELUBWD_FP8}[form], nbytes, 2 * (M // 128) if opts & COLPART else 0)


def old_ln(M, N, K, form, fp8, opts):                   # ln_launch_check's shape half + gemm_ln.hip / gemm_fp8_ln.hip
    if M % 1024 or K % (128 if fp8 else 64) or M <= 0 or N <= 0 or K <= 0:
        return refused(3)
    tile = 384 if N % 384 == 0 else 256 if N % 256 == 0 else 0
    if not tile or N // tile > 4:
        return refused(3)
    if fp8:
        nbytes = (M * K + N * K) + M * N * 4 + (2.0 * M * N if opts & RES else 0.0) + (M * N if opts & C8 else 0.0)
        cls = K_LNFWD_FP8 if form == LNFWD else K_LNBWD_FP8
    else:
        nbytes = 2.0 * (M * K + N * K) + M * N * 4 + (2.0 * M * N if opts & RES else 0.0)
        cls = K_LNFWD if form == LNFWD else K_LNBWD
    # mode 6 requires colpart and writes [2 * M / 128][3][N]; mode 5 has no column sums
    return pipeline(M, N, K, 384 if tile == 384 else 1256, 1, cls, nbytes, 2 * (M // 128) if form == LNBWD else 0)


def old_gelud(M, N, K, form, fp8, opts):                # the two derivative-stash launchers
    if fp8:
        if M % 128 or N % 256 or K % 128 or M <= 0 or N <= 0 or K <= 0:
            return refused(3)
        tm = 256 if M % 256 == 0 else 128               # plb_gemm_nt_fp8_gelud_tile_rows
        nbytes = (M * K + N * K) + 2.0 * M * N + (2.0 * M * N if opts & OUT16 else 0.0) + (M * N if opts & C8 else 0.0)
        cls = K_GELUBWD_FP8 if form == GELUDBWD else K_GELU_FP8
    else:
        if M % 256 or N % 256 or K % 64 or M <= 0 or N <= 0 or K <= 0:
            return refused(3)
        tm = 256
        nbytes = 2.0 * (M * K + N * K) + 4.0 * M * N
        cls = K_GELUBWD if form == GELUDBWD else K_GELU
    return pipeline(M, N, K, 256 if tm == 256 else 1256, 1, cls, nbytes, 2 * (M // tm) if opts & COLPART else 0)


def old_rules(M, N, K, form, ops, opts, g_tile=0, g_pf=-1):
    fp8 = ops != BF16
    if form in (LNFWD, LNBWD):
        return old_ln(M, N, K, form, fp8, opts)
    if form in (GELUD, GELUDBWD):
        return old_gelud(M, N, K, form, fp8, opts)
    if fp8:   # no fp8 launcher took fp32 out or the cross-entropy passes: the plan refuses them
        return old_fp8(M, N, K, form, opts) if form in (PLAIN, GELU, GELUBWD) else refused(1)
    if form in (CE1, CE2):
        return old_token_head(M, N, K, form, opts, g_pf)
    return old_launch_gemm_nt(M, N, K, form, opts, g_tile, g_pf)


def shapes():
    return list(itertools.product(MS, NS, KS)) + EXTRA


def same(got, want, what):
    assert got == want, f"{what}: plan {got}, the launchers' rules {want}"


def test_every_form_operand_kind_and_shape():
    L = _lib.lib()
    n = 0
    for (M, N, K), form, ops in itertools.product(shapes(), range(10), (BF16, E4M3, E5M2)):
        for opts in (0, COLPART, RES | C8 | OUT16, COLPART | RES | C8 | OUT16):
            same(plan(L, M, N, K, form, ops, opts), old_rules(M, N, K, form, ops, opts), (M, N, K, form, ops, opts))
            n += 1
    assert n == (14 * 16 * 5 + len(EXTRA)) * 10 * 3 * 4


def test_the_edges_the_rules_turn_on():
    L = _lib.lib()
    # the small-problem edge of pick_tile: M N < 256 * 256 * 64 goes to the small kernel
    assert 2048 * 1536 < 256 * 256 * 64 == 2048 * 2048
    assert plan(L, 2048, 1536, 64, PLAIN, BF16, 0)["family"] == 0 and plan(L, 2048, 2048, 64, PLAIN, BF16, 0)["family"] == 1
    assert plan(L, 2048, 1536, 64, PLAIN, BF16, COLPART)["rc"] == 1            # colpart on a shape of the small kernel
    # the 64x64 rule: fewer than 256 workgroups of 128x128
    for M, N, grid128 in ((32640, 124, 255), (1920, 2176, 255), (32768, 124, 256)):
        assert (M // 128) * ((N + 127) // 128) == grid128
        p = plan(L, M, N, 64, PLAIN, BF16, 0)
        assert (p["family"], p["tile"]) == (0, 64 if grid128 < 256 else 128), (M, N, p)
    # the LayerNorm forms: at most 4 column tiles, 3 before 1
    for N, rc in ((1024, 0), (1280, 3), (1536, 0), (1920, 3)):
        for ops in (BF16, E4M3, E5M2):
            assert plan(L, 1024, N, 128, LNFWD, ops, 0)["rc"] == rc and plan(L, 1024, N, 128, LNBWD, ops, 0)["rc"] == rc
    assert plan(L, 1024, 768, 128, LNBWD, BF16, 0)["colpart_rows"] == 16 and plan(L, 1024, 768, 128, LNFWD, BF16, COLPART)["colpart_rows"] == 0
    # a form or an operand kind that does not exist
    assert plan(L, 1024, 768, 128, 10, BF16, 0)["rc"] == 1 and plan(L, 1024, 768, 128, -1, BF16, 0)["rc"] == 1
    assert plan(L, 1024, 768, 128, PLAIN, 3, 0)["rc"] == 1


@pytest.fixture
def tuning():
    L = _lib.lib()
    yield L
    L.plb_set_gemm_nt_tile(0)
    L.plb_set_gemm_nt_prefetch(-1)


def test_plain_forms_under_the_tuning_hooks(tuning):
    L = tuning
    for g_tile, g_pf in itertools.product((0, 64, -64, 128, 256, 384, 1256), (-1, 0, 1)):
        L.plb_set_gemm_nt_tile(g_tile)
        L.plb_set_gemm_nt_prefetch(g_pf)
        for (M, N, K), form, opts in itertools.product(shapes(), (PLAIN, GELU, GELUBWD, F32), (0, COLPART)):
            same(plan(L, M, N, K, form, BF16, opts), old_rules(M, N, K, form, BF16, opts, g_tile, g_pf), (M, N, K, form, opts, g_tile, g_pf))
        # the forms that have one K loop only, and the fp8 forms, do not look at the hooks
        for form, ops in ((LNFWD, BF16), (LNBWD, E5M2), (GELUD, BF16), (GELUDBWD, E5M2), (PLAIN, E4M3), (GELU, E4M3)):
            same(plan(L, 2048, 768, 768, form, ops, COLPART), old_rules(2048, 768, 768, form, ops, COLPART), (form, ops, g_tile, g_pf))


def test_the_callers_tile_of_the_pipeline_launcher(tuning):
    """plb_launch_gemm_nt_big runs the tile its caller names: the shape lines of launch_big (1, never 3), 256-column tiles
    for the cross-entropy passes, the K-loop rule, and no look at plb_set_gemm_nt_tile."""
    L = tuning
    for g_tile, g_pf in ((0, -1), (128, 0), (384, 1)):
        L.plb_set_gemm_nt_tile(g_tile)
        L.plb_set_gemm_nt_prefetch(g_pf)
        for (M, N, K), tile, form, opts in itertools.product(shapes(), (256, 384, 1256), (PLAIN, GELU, GELUBWD, CE1, CE2, F32), (0, COLPART)):
            same(plan(L, M, N, K, form, BF16, opts, tile), old_launch_big(M, N, K, tile, form, opts, g_pf), (M, N, K, tile, form, opts, g_pf))
    for form, ops in ((LNFWD, BF16), (GELUD, BF16), (PLAIN, E4M3), (CE1, E4M3)):   # forms and operands that launcher never had
        assert plan(L, 2048, 768, 768, form, ops, 0, 256)["rc"] == 1


def test_the_wrappers_are_the_plan(tuning):
    L = tuning
    for g_tile in (0, 128, 256, 384, 1256):
        L.plb_set_gemm_nt_tile(g_tile)
        for M, N, K in shapes():
            p = plan(L, M, N, K, PLAIN, BF16, COLPART)
            rows = L.plb_gemm_nt_colpart_rows(M, N, K)
            assert rows == (0 if p["rc"] else p["colpart_rows"])
            tile = pick_tile(M, N, g_tile)                                   # what the function returned before
            assert rows == (2 * (M // 256) if tile == 256 else 2 * (M // 128) if tile in (384, 1256) else 0), (M, N, K, g_tile)
    L.plb_set_gemm_nt_tile(0)
    for M in MS + [100]:
        p = plan(L, M, 256, 128, GELUD, E4M3, 0)
        assert L.plb_gemm_nt_fp8_gelud_tile_rows(M) == (128 if p["rc"] else p["tile_m"]) == (256 if M % 256 == 0 else 128), M


SWEEP_MAIN = r"""
#include <cstdio>
#include <initializer_list>
#include "gemm_nt_plan.h"
extern "C" void plb_set_gemm_nt_tile(int), plb_set_gemm_nt_prefetch(int);
int main() {
  const int Ms[] = {-128, 0, 64, 128, 192, 256, 384, 512, 1024, 1920, 2048, 2304, 3072, 8192, 16384, 32640, 32768, 49152, 2147483520};
  const int Ns[] = {-4, 0, 4, 124, 128, 188, 256, 384, 512, 768, 1024, 1280, 1536, 1920, 2048, 2176, 2304, 3072, 4096, 5120, 64000, 2147483392};
  const int Ks[] = {0, 64, 128, 192, 768, 2048};
  const int tiles[] = {0, 64, -64, 128, 256, 384, 1256};
  long runs = 0, sum = 0;
  for (int i = 0; i < 7; ++i) {
    plb_set_gemm_nt_tile(tiles[i]); plb_set_gemm_nt_prefetch(i % 3 - 1);
    for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int form = -1; form <= 10; ++form) for (int ops = 0; ops < 3; ++ops)
      for (int opts = 0; opts < 16; opts += 15) for (int tile : {0, 256, 384, 1256, 7}) {
        PlbGemmNTPlan p;
        const int rc = plb_gemm_nt_plan(M, N, K, form, ops, opts, tile, &p);
        if (rc != p.rc || (rc && (p.grid || p.colpart_rows || p.bytes != 0)) || (!rc && (p.grid <= 0 || p.block <= 0 || p.colpart_rows < 0))) {
          printf("inconsistent plan at %d %d %d form %d ops %d opts %d tile %d\n", M, N, K, form, ops, opts, tile);
          return 1;
        }
        runs += rc == 0; sum += (long)p.grid + p.colpart_rows;
      }
  }
  printf("plans that run: %ld, checksum %ld\n", runs, sum);
  return 0;
}
"""


def test_the_plan_unit_under_address_and_ub_sanitizers(tmp_path):
    """The unit is plain C++ with no HIP header: compiled with the host compiler and a main of its own, instrumented, and
    run as a program (shapes beyond the grid of this file included: zero, negative and near 2^31)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "plbert_amd", "csrc")
    (tmp_path / "main.cpp").write_text(SWEEP_MAIN)
    exe = tmp_path / "plan_sweep"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", csrc, os.path.join(csrc, "gemm_nt_plan.cpp"), str(tmp_path / "main.cpp"), "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0 and "plans that run" in r.stdout, r.stdout[-3000:]
