"""What key masks cost the attention kernels: python tools/keymask_bench.py [--rounds 9] [--iters 20] [--out FILE]

Attention forward + backward (plb_launch_attn_fwd + plb_launch_attn_bwd, two-kernel form in both arms: a call with words
always takes it) at 32 x 512 x 12 heads, the step's shape. Each case alternates the call WITHOUT words with the call WITH
them, on the same qkv / dctx:

 ones     all-ones mask                against lengths = NULL          (the same work: what the masked K loop itself adds)
 leftpad  left pad of 25 % (128 keys)  against the right-padded batch, lengths = 384 (the same valid keys; the masked call
                                       still runs all 8 key tiles of every query tile and skips the arithmetic of the empty two)
 random   Bernoulli(0.9) mask          against lengths = NULL          (every tile takes the select arm)

One timed run = `iters` forward + backward pairs between two device events; `rounds` alternated runs per arm after two
warm-up runs of each; medians, minima, the ratio of the medians; then, with the per-launch event profiler on, the time per
launch of each kernel class in each arm. Prints a table, then one JSON line; --out appends both."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from plbert_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, S, NH = a.batch, a.seq, a.heads
    H = NH * 64
    dev = "cuda"
    L = _lib.lib()
    L.plb_set_attn_bwd_fused(0)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B * S, 3 * H, generator=g).to(torch.bfloat16).to(dev)
    dctx = torch.randn(B * S, H, generator=g).to(torch.bfloat16).to(dev)
    ctx = torch.zeros((B * S, H), dtype=torch.bfloat16, device=dev)
    # csrc/attn_plan.h: the statistics' size, and the form a call with words gets whatever the policy says
    plan = _lib.attn_plan(B, S, NH, _lib.ATTN_KEYMASK | _lib.ATTN_OUT_ROWS)
    assert plan["rc"] == 0 and plan["bwd_form"] == 0 and plan["km"] == 1, plan
    lse = torch.zeros(plan["stat_floats"], dtype=torch.float32, device=dev)
    delta = torch.zeros(plan["stat_floats"], dtype=torch.float32, device=dev)
    dqkv = torch.zeros((B * S, 3 * H), dtype=torch.bfloat16, device=dev)
    ldkw = 2 * ((S + 63) // 64)

    def words(mask, lengths):
        w = torch.zeros(B * ldkw, dtype=torch.int32, device=dev)
        rc = L.plb_launch_key_mask_words(mask.data_ptr(), None if lengths is None else lengths.data_ptr(), B, S, w.data_ptr(),
                                         ldkw, stream())
        assert rc == 0
        return w

    def call(lengths, w):
        p = _lib.PlbAttn()
        p.qkv, p.ldqkv, p.B, p.S, p.NH, p.H, p.scale = qkv.data_ptr(), 3 * H, B, S, NH, H, 0.125
        p.lengths = None if lengths is None else lengths.data_ptr()
        p.ctx, p.ldctx, p.lse = ctx.data_ptr(), H, lse.data_ptr()
        p.dctx, p.lddctx, p.delta, p.dqkv, p.lddqkv = dctx.data_ptr(), H, delta.data_ptr(), dqkv.data_ptr(), 3 * H
        if w is not None:
            p.key_words, p.ldkw = w.data_ptr(), ldkw

        def run():
            for _ in range(a.iters):
                assert L.plb_launch_attn_fwd(C.byref(p), stream()) == 0
                assert L.plb_launch_attn_bwd(C.byref(p), stream()) == 0
        return run

    ones = torch.ones(B, S, dtype=torch.int32, device=dev)
    left = ones.clone()
    left[:, :S // 4] = 0
    rnd = (torch.rand(B, S, generator=g) < 0.9).to(torch.int32).to(dev)
    rnd[:, -1] = 1
    short = torch.full((B,), S - S // 4, dtype=torch.int32, device=dev)
    cases = {
        "ones": (call(None, None), call(None, words(ones, None))),
        "leftpad": (call(short, None), call(None, words(left, None))),
        "random": (call(None, None), call(None, words(rnd, None))),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters   # us per forward + backward pair

    res = {"shape": [B, S, NH], "iters": a.iters, "rounds": a.rounds}
    lines = [f"attention forward + backward, {B} x {S} x {NH} heads, us per pair (median | min), {a.rounds} alternated runs of "
             f"{a.iters} pairs"]
    for name, (plain, masked) in cases.items():
        for _ in range(2):
            timed(plain), timed(masked)
        tp, tm = [], []
        for _ in range(a.rounds):
            tp.append(timed(plain))
            tm.append(timed(masked))
        mp, mm = statistics.median(tp), statistics.median(tm)
        res[name] = {"plain_us": round(mp, 2), "plain_min_us": round(min(tp), 2), "masked_us": round(mm, 2),
                     "masked_min_us": round(min(tm), 2), "ratio": round(mm / mp, 4),
                     "plain_spread": round((max(tp) - min(tp)) / mp, 4)}
        lines.append(f" {name:8s} without words {mp:8.2f} | {min(tp):8.2f}   with words {mm:8.2f} | {min(tm):8.2f}   ratio "
                     f"{mm / mp:.4f}   (spread of the runs without words: {res[name]['plain_spread']:.4f})")
    # per kernel, in a pass of its own with the per-launch event profiler on (the figures above are taken with it off)
    _lib.profile_enable(True)
    split = {}
    for name, (plain, masked) in cases.items():
        for arm, fn in (("without", plain), ("with", masked)):
            timed(fn)
            _lib.profile_read()
            timed(fn)
            rd = _lib.profile_read()
            split[f"{name}_{arm}"] = {k: round(v["ms"] * 1e3 / v["launches"], 2) for k, v in rd.items()}
            lines.append(f" {name:8s} {arm:7s} words, us per launch: " + ", ".join(f"{k} {v}" for k, v in split[f"{name}_{arm}"].items()))
    _lib.profile_enable(False)
    res["per_kernel_us"] = split
    L.plb_set_attn_bwd_fused(-1)
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
