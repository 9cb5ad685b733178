"""Micro-benchmark of the NT / TN GEMM kernels through the C ABI (run on the GPU box).
   python tools/gemm_bench.py [--tiles 128,256]"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from plbert_amd import _lib  # noqa: E402

SHAPES = [(16384, 768, 768), (16384, 2304, 768), (16384, 2048, 768), (16384, 768, 2048), (16384, 768, 2304),
          (8192, 8192, 8192), (4096, 4096, 4096)]


MSTORE_ZERO = False
WITH_RES = False

# The launches of the small NT kernel in the bench step (--small-ab): (label, N, K, act, residual, fp32 output). The compact
# rows of the pruned last application: dense, FFN up (gelu), FFN output forward; their three dX products backward.
SMALL_COMPACT = [("dense fwd", 768, 768, 0, True, False), ("ffn fwd gelu", 2048, 768, 1, False, False),
                 ("ffn_out fwd", 768, 2048, 0, True, False), ("ffn_out dX", 2048, 768, 2, False, False),
                 ("ffn dX", 768, 2048, 0, False, False), ("dense dX", 768, 768, 0, False, False)]
SMALL_AB = ([(f"{n} M{M}", M, N, K, a, r, f) for M in (1920, 2048) for (n, N, K, a, r, f) in SMALL_COMPACT] +
            [("head logits", 2048, 180, 768, 0, False, True), ("head dH", 2048, 768, 256, 0, False, False),
             ("map-in dE", 16384, 128, 768, 0, False, False)])


def time_nt(L, M, N, K, act, iters=20, res=None, out_f32=0):
    dev = "cuda"
    A = (torch.randn(M, K, device=dev)).to(torch.bfloat16)
    B = (torch.randn((N + 127) // 128 * 128, K, device=dev) * 0.05).to(torch.bfloat16)  # the kernels read whole tiles of B rows
    Cb = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    C2 = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    bias = torch.randn(N, device=dev)
    p = _lib.PlbGemmNT()
    p.A, p.lda, p.B, p.ldb, p.M, p.N, p.K, p.Mstore = A.data_ptr(), K, B.data_ptr(), K, M, N, K, (0 if MSTORE_ZERO else M)
    p.bias = bias.data_ptr()
    p.C, p.ldc, p.C2, p.ldc2 = Cb.data_ptr(), N, C2.data_ptr(), N
    if out_f32:
        Cf = torch.empty(M, 256, dtype=torch.float32, device=dev)
        p.Cf, p.ldcf = Cf.data_ptr(), 256
    if WITH_RES if res is None else res:
        R = torch.randn(M, N, device=dev).to(torch.bfloat16)
        p.res, p.ldr = R.data_ptr(), N
    if act == 2:
        U = torch.randn(M, N, device=dev).to(torch.bfloat16)
        p.aux, p.ldaux = U.data_ptr(), N
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        assert L.plb_launch_gemm_nt(C.byref(p), act, out_f32, s) == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        L.plb_launch_gemm_nt(C.byref(p), act, out_f32, s)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    return ms, 2.0 * M * N * K / (ms * 1e-3) / 1e12


TN_SHAPES = [(196608, 2304, 768), (196608, 768, 768), (196608, 2048, 768), (196608, 768, 2048),
             (16384, 2304, 768), (16384, 768, 768), (32768, 2304, 768)]


def time_tn(L, Mtot, N, K, kind, iters=5):
    """kind "bf16": the kernel the plan picks for the shape (pipeline or small); "fp8": the pipeline kernel on 1-byte images
    with unit dequantisation factors. Splits and rows per split are the plan's (csrc/gemm_tn_plan.h), i.e. the engine's."""
    dev = "cuda"
    fp8 = kind == "fp8"
    pl = _lib.gemm_tn_plan(Mtot, N, N, K, int(fp8))
    assert pl["rc"] == 0, (Mtot, N, K, kind)
    if fp8:
        A = torch.randint(0, 256, (Mtot, N), dtype=torch.uint8, device=dev) & 0x77   # finite in e5m2 and e4m3
        B = torch.randint(0, 256, (Mtot, K), dtype=torch.uint8, device=dev) & 0x77
        deq = torch.ones(2, dtype=torch.float32, device=dev)
    else:
        A = torch.randn(Mtot, N, device=dev).to(torch.bfloat16)
        B = torch.randn(Mtot, K, device=dev).to(torch.bfloat16)
    splits, rps = pl["splits"], pl["rows_per_split"]
    slab = torch.empty(splits * N * K, dtype=torch.float32, device=dev)
    p = _lib.PlbGemmTN()
    p.A, p.lda, p.Ncols, p.B, p.ldb = A.data_ptr(), N, N, B.data_ptr(), K
    p.Mtot, p.N, p.K, p.rows_per_split, p.splits, p.slab = Mtot, N, K, rps, splits, slab.data_ptr()
    if fp8:
        p.deq_a, p.deq_b = deq.data_ptr(), deq.data_ptr() + 4
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = (L.plb_launch_gemm_tn, L.plb_launch_gemm_tn_big, L.plb_launch_gemm_tn_fp8)[pl["kernel"]]
    assert fn(C.byref(p), s) == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(C.byref(p), s)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    return ms, 2.0 * Mtot * N * K / (ms * 1e-3) / 1e12, splits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", default="128,256,384,0")
    ap.add_argument("--act", type=int, default=0)
    ap.add_argument("--tn", action="store_true")
    ap.add_argument("--tn-kinds", default="bf16,fp8", help="--tn: operand kinds to time (the plan picks kernel and splits)")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--small-ab", action="store_true",
                    help="the step's small-kernel launches in the 128x128 form (tile -64) and the 64x64 form (tile 64)")
    ap.add_argument("--shapes", default="", help="M,N,K;M,N,K;... instead of the built-in NT list")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--libs", default="", help="other builds of libplbert_hip.so to time beside the product build")
    ap.add_argument("--prefetch", default="-1", help="comma list of 0/1: NT big-tile K-loop variants to time")
    ap.add_argument("--res", action="store_true", help="add a bf16 residual operand in the epilogue")
    ap.add_argument("--nostore", action="store_true", help="Mstore = 0: the epilogue computes but stores nothing")
    args = ap.parse_args()
    global MSTORE_ZERO, WITH_RES
    MSTORE_ZERO = args.nostore
    WITH_RES = args.res
    L = _lib.lib()
    if args.small_ab:
        time_nt(L, *SHAPES[0], 0)  # warm the clocks
        res = {}
        for rep in range(args.reps):
            for (label, M, N, K, act, r, f32) in SMALL_AB:
                for tile in (-64, 64):
                    L.plb_set_gemm_nt_tile(tile)
                    ms, _ = time_nt(L, M, N, K, act, iters=50, res=r, out_f32=int(f32))
                    res.setdefault((label, M, N, K, tile), []).append(ms)
        L.plb_set_gemm_nt_tile(0)
        for (label, M, N, K, tile), v in res.items():
            v = sorted(v)
            print(f"{label:20s} M {M:6d} N {N:5d} K {K:5d}  form {abs(tile) if tile > 0 else 128:4d}  min {v[0]*1e3:7.2f} us  "
                  f"median {v[len(v) // 2]*1e3:7.2f} us  max {v[-1]*1e3:7.2f} us", flush=True)
        return
    if args.tn:
        libs = [("main", L)] + [(os.path.basename(q), _lib.declare(C.CDLL(os.path.abspath(q), mode=C.RTLD_LOCAL)))
                                for q in args.libs.split(",") if q]
        res = {}
        shapes_tn = TN_SHAPES[:2] if args.quick else TN_SHAPES[4:] if args.small else TN_SHAPES
        for rep in range(args.reps):
            for (M, N, K) in shapes_tn:
                for (ln, lib) in libs:
                    for kind in args.tn_kinds.split(","):
                        ms, tf, sp = time_tn(lib, M, N, K, kind, iters=3)
                        res.setdefault((ln, kind, M, N, K, sp), []).append(ms)
        for (ln, kind, M, N, K, sp), v in res.items():
            v = sorted(v)
            med = v[len(v) // 2]
            print(f"{ln:14s} tn {kind:4s} Mtot {M} N {N:5d} K {K:5d} splits {sp:3d}  median {med*1e3:9.1f} us  min {v[0]*1e3:9.1f} us  "
                  f"max {v[-1]*1e3:9.1f} us  {2.0*M*N*K/(med*1e-3)/1e12:7.1f} TFLOP/s", flush=True)
        return
    shapes = [tuple(int(v) for v in t.split(",")) for t in args.shapes.split(";")] if args.shapes else SHAPES
    # A/B protocol: box-to-box and minute-to-minute drift is 5-10 %, so variants are timed round-robin
    # inside one process (other builds of the library: --libs a.so,b.so) and the median / min over --reps
    # rounds is reported per variant.
    libs = [("main", L)]
    for path in [q for q in args.libs.split(",") if q]:
        libs.append((os.path.basename(path), _lib.declare(C.CDLL(os.path.abspath(path), mode=C.RTLD_LOCAL))))
    variants = [(ln, lib, pf, tile) for (ln, lib) in libs for pf in [int(t) for t in args.prefetch.split(",")]
                for tile in [int(t) for t in args.tiles.split(",")]]
    time_nt(L, *SHAPES[0], args.act)  # warm the clocks
    res = {}
    for rep in range(args.reps):
        for (M, N, K) in shapes:
            for (ln, lib, pf, tile) in variants:
                lib.plb_set_gemm_nt_prefetch(pf)
                lib.plb_set_gemm_nt_tile(tile)
                ms, tf = time_nt(lib, M, N, K, args.act)
                res.setdefault((ln, pf, tile, M, N, K), []).append(ms)
    for (ln, pf, tile, M, N, K), v in res.items():
        v = sorted(v)
        med = v[len(v) // 2]
        print(f"{ln:14s} pf {pf:2d} tile {tile:4d}  M {M:6d} N {N:5d} K {K:5d}  median {med*1e3:8.1f} us  min {v[0]*1e3:8.1f} us"
              f"  {2.0*M*N*K/(med*1e-3)/1e12:7.1f} TFLOP/s", flush=True)

if __name__ == "__main__":
    main()
