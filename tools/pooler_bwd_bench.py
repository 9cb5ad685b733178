"""What a gradient of pooler_output costs the fine-tuning pair, on ONE box in ONE process (a tool, not a test; bench.py
measures the pre-training step only). Config A (768 / 12 layers / 12 heads / FFN 2048), bf16, 32 x 512, bench.py's seeded
full-length batch (synthetic_batch(32, 512, seed=1234)):
  plain  : plb_encode + plb_encode_bwd (a resident seeded d_hidden)
  pooled : plb_encode + plb_encode_bwd_pooled (the same d_hidden and a resident d_pooled): four small launches more — dpre,
           dW | db, dh0 (pooler_bwd.hip) and the seed of the B first rows — and 2.4 MB more in the head piece of an exchange.
The legs ALTERNATE in blocks of --steps timed pairs (device events around every pair, after --warmup pairs of each leg),
--reps blocks per leg; the spread printed is the range of the block medians of one leg, i.e. what the same code does from
block to block on this box. No optimizer step: the pair is the subject (the update of the pooler's 0.6 M floats rides on the
encoder's 11 M).
   python tools/pooler_bwd_bench.py [--reps 5] [--steps 20] [--warmup 5] [--out profiles/pooler_bwd_ab.txt]"""
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
    ap.add_argument("--out", default=None, help="append the summary to this file")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import plbert_amd
    from plbert_amd.engine import HipEngine

    if not torch.cuda.is_available():
        raise SystemExit("pooler_bwd_bench needs the GPU: a timing taken anywhere else says nothing")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    pcfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                   num_hidden_layers=12, max_position_embeddings=512)
    _, masked, _, _ = plbert_amd.synthetic_batch(32, 512, seed=1234)
    B, S = masked.shape
    eng = HipEngine(pcfg, 188, 0, max_batch=B, max_seq=S)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(pcfg, 188, seed=0))
    ids_d = eng._dev_i64(masked)
    gen = torch.Generator("cuda").manual_seed(5)
    d_hidden = torch.randn((B, S, pcfg.hidden_size), device="cuda:0", generator=gen) * 1e-2
    d_pooled = torch.randn((B, pcfg.hidden_size), device="cuda:0", generator=gen)

    def plain():
        eng.encode(ids_d, None)
        eng.encode_bwd(d_hidden)

    def pooled():
        eng.encode(ids_d, None)
        eng.encode_bwd(d_hidden, d_pooled=d_pooled)

    legs = {"plain": plain, "pooled": pooled}
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
    assert eng.status()["ln_exchange_timeouts"] == 0
    say(f"encode + encode_bwd, config A, 32 x 512, {a.reps} blocks of {a.steps} pairs per leg, ms per pair:")
    for name, m in meds.items():
        say(f"  {name:7s} median {statistics.median(m):8.3f}  blocks {', '.join(f'{x:.3f}' for x in m)}  spread {max(m) - min(m):.3f}")
    diff = statistics.median(meds["pooled"]) - statistics.median(meds["plain"])
    spread = max(max(m) - min(m) for m in meds.values())
    say(f"  pooled - plain = {diff:+.3f} ms (largest block-to-block spread {spread:.3f} ms)")
    say("  " + json.dumps({**{k: round(statistics.median(v), 4) for k, v in meds.items()}, "delta_ms": round(diff, 4),
                           "spread_ms": round(spread, 4)}))
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
