"""Padded against token-packed training steps on a RAGGED batch, on ONE box (bench.py measures the resident full-length
batch, where packing has nothing to remove). The batch is the reference-captured fixture tests/golden/real_s512_b32_ragged
(32 x 512, lengths 512 .. 74: 10,271 valid tokens of 16,384 rows) at config A (768 / 12 layers / 12 heads / FFN 2048), one
training step = loss + backward + AdamW on the resident batch; a full-length 32 x 512 batch is the control (a plan of
full lengths is the padded layout: that leg shows what the packed entry point costs when it has nothing to do, and the
box's run-to-run spread).
Every measurement is a fresh child process under its own time limit, variants round-robin; the parent never opens the
GPU.
   python tools/ragged_bench.py [--reps 3] [--steps 30] [--warmup 10] [--timeout 300] label[:ENV=VAL[,ENV=VAL...]] ...
e.g. python tools/ragged_bench.py parent:PLBERT_HIP_LIB=plbert_amd/build/ab/lib_parent.so,PACKED=0 padded:PACKED=0 packed
PACKED=0 in a variant's list: padded calls only (a library built before the packed entry points existed has no others);
the default variant runs both legs, packed and padded.  Prints one JSON line per child and a summary with ms/step and
VALID tokens/s (the batch's real tokens per second: the figure that packing can move).
--num-tokens N: the DUAL-HEAD step with a token head of N classes (the ragged fixture has no token ids: they are drawn
from a fixed seed). The packed leg then runs with plb_set_packed_dual on, and a third leg, switch_off, hands the same plan
to a trainer with the switch off (it must run padded: the control of the opt-in). A library that predates the switch takes
PACKED=0 as before. One leg under a profiler:
   rocprofv3 --kernel-trace --stats -d DIR -- python tools/ragged_bench.py --child --num-tokens 64000 --steps 20 --legs packed
e.g. python tools/ragged_bench.py --num-tokens 64000 parent:PLBERT_HIP_LIB=plbert_amd/build/ab/lib_parent.so,PACKED=0 here
--dtype fp8: every leg trains in fp8 mode (plb_set_fp8; the warm-up holds the calibration call). Three legs: padded (no
plan), packed (plan + plb_set_packed_fp8 on) and switch_off (plan, switch off: it must run padded — the parent's code path
with a plan in hand). --profile adds the per-class launch times of plb_profile_read (ms per step) of a few extra steps after
the timed ones. The summary gives, per leg, the spread of its runs ((max - min) / median)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from conftest import golden_cfg, load_golden
    import plbert_amd
    from plbert_amd.train import PLBertTrainer

    g = load_golden("real_s512_b32_ragged")
    _, pcfg, sd = golden_cfg(g)
    B, S = g["labels"].shape
    legs = {}
    if a.batch == "ragged":
        labels, masked = g["labels"], g["masked"]
        lengths, idx = [int(x) for x in g["lengths"]], [list(map(int, x)) for x in g["index"]]
    else:
        labels, masked, lengths, idx = plbert_amd.synthetic_batch(B, S, seed=1234)
        lengths = [S] * B
    valid = int(np.sum(lengths))
    NT = a.num_tokens
    tok = None
    if NT:   # dual-head step: token targets from a fixed seed, the reference's initialisation with the second head
        tok = np.random.RandomState(4321).randint(0, NT, size=(B, S)).astype(np.int64)
        sd = plbert_amd.reference_init_state_dict(pcfg, int(g["num_phonemes"]), NT, seed=0)
    f8 = a.dtype == "fp8"
    names = ["padded"] + (["packed"] + (["switch_off"] if NT or f8 else []) if a.packed else [])
    if a.legs:   # (one leg alone: a profiler run of a --child process)
        names = [n for n in names if n in a.legs.split(",")]
    for leg in names:
        packed = leg != "padded"
        kw = {"packed": True} if packed else {}
        tkw = dict(kw, num_tokens=NT, **({"packed_dual": leg == "packed"} if packed else {})) if NT else dict(kw)
        if f8 and packed:   # (fp8 + dual head: the packed leg turns both switches on, switch_off neither)
            tkw["packed_fp8"] = leg == "packed"
        tr = PLBertTrainer(pcfg, int(g["num_phonemes"]), max_batch=B, max_seq=S, lr=7e-5, device="cuda:0", state_dict=sd, **tkw)
        if f8:
            tr.engine.set_fp8(True)
        batch = tr.stage_batch(labels, masked, lengths, idx, token_ids=tok, **kw)
        for _ in range(a.warmup):
            tr.step(batch)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
        ev[0].record()
        for i in range(a.steps):
            loss = tr.step(batch)
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps))
        med = ms[len(ms) // 2]
        rows = tr.engine.last_call_rows() if packed else (B * S, B * S)
        legs[leg] = {
            "ms_per_step": round(med, 4), "ms_min": round(ms[0], 4), "ms_p90": round(ms[int(0.9 * (len(ms) - 1))], 4),
            "valid_tokens_per_s": round(valid / med * 1e3, 1), "rows": int(rows[0]), "of": int(rows[1]),
            "loss": float(loss.item()), "timeouts": tr.engine.status()["ln_exchange_timeouts"]}
        if f8:
            legs[leg]["fp8_calibrated"] = bool(tr.engine.fp8_state()[1])
        if a.profile:   # per-class launch times, outside the timed steps (the profiler's events cost time of their own)
            from plbert_amd import _lib
            nprof = 5
            _lib.profile_enable(True)
            _lib.profile_read()
            for _ in range(nprof):
                tr.step(batch)
            torch.cuda.synchronize()
            legs[leg]["profile_ms_per_step"] = {k: round(v["ms"] / nprof, 4) for k, v in _lib.profile_read().items()}
            _lib.profile_enable(False)
        del tr
    print(json.dumps({"batch": a.batch, "valid_tokens": valid, "legs": legs}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--batch", choices=["ragged", "full"], default="ragged")
    ap.add_argument("--packed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=300, help="seconds, per child process")
    ap.add_argument("--legs", default="", help="with --child: run these legs only (padded,packed,switch_off)")
    ap.add_argument("--num-tokens", type=int, default=0, help="dual-head step with a token head of this many classes")
    ap.add_argument("--dtype", choices=["bf16", "fp8"], default="bf16", help="fp8: every leg in fp8 mode (plb_set_fp8)")
    ap.add_argument("--profile", action="store_true", help="add plb_profile_read's per-class ms per step to every leg")
    ap.add_argument("variants", nargs="*", default=["here"])
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {}
    for rep in range(a.reps):
        for batch in ("ragged", "full"):
            for v in a.variants:
                label, _, envs = v.partition(":")
                env, packed = dict(os.environ), 1
                env.pop("PLBERT_PACKED", None)
                env.pop("PLBERT_PACKED_DUAL", None)
                env.pop("PLBERT_PACKED_FP8", None)
                for kv in [e for e in envs.split(",") if e]:
                    k, _, val = kv.partition("=")
                    if k == "PACKED":
                        packed = int(val)
                    else:
                        env[k] = os.path.abspath(os.path.join(ROOT, val)) if k == "PLBERT_HIP_LIB" else val
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batch", batch, "--packed", str(packed),
                       "--steps", str(a.steps), "--warmup", str(a.warmup), "--num-tokens", str(a.num_tokens), "--dtype", a.dtype] + (["--profile"] if a.profile else [])
                try:
                    out = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=a.timeout)
                except subprocess.TimeoutExpired:
                    print(f"{label} {batch}: no result within {a.timeout} s; stopping", flush=True)
                    return 1
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
                if out.returncode != 0 or not line:   # nothing more is started on a GPU that has just failed a run
                    print(f"{label} {batch}: FAILED (exit {out.returncode})\n{out.stderr[-800:]}", flush=True)
                    return 1
                d = json.loads(line[-1])
                print(json.dumps({"variant": label, "rep": rep, **d}), flush=True)
                for leg, r in d["legs"].items():
                    res.setdefault((batch, label, leg), []).append(r)
    print("--- median over the runs: ms/step (all runs) | valid tokens/s | rows executed | spread of the runs")
    med = {}
    for (batch, label, leg), rs in res.items():
        ms = [r["ms_per_step"] for r in rs]
        med[(batch, label, leg)] = statistics.median(ms)
        print(f"{batch:7s} {label:10s} {leg:10s} {statistics.median(ms):8.3f} ({', '.join(f'{x:.3f}' for x in ms)}) | "
              f"{statistics.median(r['valid_tokens_per_s'] for r in rs):10.0f} | {rs[0]['rows']} of {rs[0]['of']} | "
              f"{100 * (max(ms) - min(ms)) / statistics.median(ms):.1f} %")
    base = a.variants[0].partition(":")[0]
    for (batch, label, leg), m in med.items():
        ref = med.get((batch, base, "padded"))
        if ref and (label, leg) != (base, "padded"):
            print(f"{batch:7s} {label}/{leg} against {base}/padded: x{ref / m:.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
