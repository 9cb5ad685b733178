"""The fine-tuning pair against the unpruned pre-training step, on ONE box in ONE process (a tool, not a test; bench.py
measures the pre-training step only). Config A (768 / 12 layers / 12 heads / FFN 2048), bf16, 32 x 512:
  finetune : plb_encode + plb_encode_bwd (a resident seeded d_hidden) + plb_adamw_step
  loss     : plb_loss_fwd_bwd with plb_set_prune_last(0) + plb_adamw_step — the same rows through the same GEMMs, plus the
             phoneme head (gather, head GEMM, cross entropy, its weight gradient), so the pair is expected to be no slower
             than this leg by more than the spread the tool reports.
Two batches: bench.py's seeded full-length batch (synthetic_batch(32, 512, seed=1234)) and the ragged fixture
tests/golden/real_s512_b32_ragged with token packing on. The legs ALTERNATE in blocks of --steps timed steps (device events
around every step, after --warmup steps of each leg), --reps blocks per leg; the spread printed is the range of the block
medians of one leg, i.e. what the same code does from block to block on this box.
   python tools/finetune_bench.py [--reps 5] [--steps 20] [--warmup 5] [--out profiles/finetune_bench.txt]
   rocprofv3 --kernel-trace --stats -d DIR -- python tools/finetune_bench.py --reps 1 --steps 5 --only full
(the second form, a run of its own: seed_dy_kernel shows as one launch per step)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["full", "ragged"], default=None)
    ap.add_argument("--out", default=None, help="append the summary to this file")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from conftest import golden_cfg, load_golden
    import plbert_amd
    from plbert_amd import _lib
    from plbert_amd.engine import HipEngine, packing_plan

    if not torch.cuda.is_available():
        raise SystemExit("finetune_bench needs the GPU: a timing taken anywhere else says nothing")
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for which in ([a.only] if a.only else ["full", "ragged"]):
        if which == "full":
            pcfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                           num_hidden_layers=12, max_position_embeddings=512)
            sd, nph = plbert_amd.deterministic_state_dict(pcfg, 188, seed=0), 188
            labels, masked, lengths, idx = plbert_amd.synthetic_batch(32, 512, seed=1234)
            lens, plan = None, None
        else:
            g = load_golden("real_s512_b32_ragged")
            _, pcfg, sd = golden_cfg(g)
            nph = int(g["num_phonemes"])
            labels, masked = g["labels"], g["masked"]
            idx = [list(map(int, x)) for x in g["index"]]
            lens = np.asarray(g["lengths"], np.int32)
            plan = packing_plan(lens, 512).to("cuda:0", non_blocking=False)
        B, S = masked.shape
        eng = HipEngine(pcfg, nph, 0, max_batch=B, max_seq=S)
        eng.load_state_dict(sd)
        off, flat = plbert_amd.masked_indices_to_csr(idx)
        n = int(off[-1])
        ids_d, lab_d = eng._dev_i64(masked), eng._dev_i64(labels)
        off_d, flat_d, lens_d = eng._dev_i32(off), eng._dev_i32(flat), eng._dev_i32(lens)
        d_hidden = torch.randn((B, S, pcfg.hidden_size), device="cuda:0", generator=torch.Generator("cuda").manual_seed(5)) * 1e-2
        step = [0]

        def finetune():
            eng.encode(ids_d, lens_d, packing=plan)
            eng.encode_bwd(d_hidden)
            step[0] += 1
            eng.adamw_step(step[0], lr=1e-5)

        def loss():
            eng.loss_fwd_bwd(ids_d, lab_d, lens_d, off_d, flat_d, n, packing=plan)
            step[0] += 1
            eng.adamw_step(step[0], lr=1e-5)

        L.plb_set_prune_last(0)
        legs = {"finetune": finetune, "loss_unpruned": loss}
        meds = {k: [] for k in legs}
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        for rep in range(a.reps):
            for name, fn in legs.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
                ev[0].record()
                for i in range(a.steps):
                    fn()
                    ev[i + 1].record()
                torch.cuda.synchronize()
                meds[name].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(a.steps)))
        L.plb_set_prune_last(-1)
        rows = eng.last_call_rows()
        assert eng.status()["ln_exchange_timeouts"] == 0
        say(f"{which} 32 x 512 ({rows[0]} rows executed of {rows[1]}), {a.reps} blocks of {a.steps} steps per leg, ms per step:")
        for name, m in meds.items():
            say(f"  {name:14s} median {statistics.median(m):8.3f}  blocks {', '.join(f'{x:.3f}' for x in m)}  "
                f"spread {max(m) - min(m):.3f}")
        diff = statistics.median(meds["finetune"]) - statistics.median(meds["loss_unpruned"])
        spread = max(max(m) - min(m) for m in meds.values())
        say(f"  finetune - loss_unpruned = {diff:+.3f} ms (largest block-to-block spread {spread:.3f} ms)")
        say("  " + json.dumps({"batch": which, **{k: round(statistics.median(v), 4) for k, v in meds.items()}, "spread_ms": round(spread, 4)}))
        del eng
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
