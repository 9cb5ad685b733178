"""The LAMB step against the grouped AdamW step at full size, on ONE box in ONE process (a tool, not a test; bench.py measures
the whole pre-training step). Bench model (768 / 12 heads / FFN 2048, 188 phonemes), without a token head and with one of
64 000 tokens (made live by one tiny dual-head loss call; both optimizers then step it as a range of its own).
  adamw : plb_adamw_step_groups, two-group recipe (no weight decay on names holding "bias" or "LayerNorm"): 1 launch per range,
          30 B per stepped float
  lamb  : plb_lamb_step, the same groups with the trust ratio off for the no-decay group: pass 1 (24 B), finish, pass 2 (18 B)
          per range
Kernel time comes from the library's own per-launch device events (plb_profile_*): class "adamw" holds the AdamW launch and
LAMB's two passes, class "reduce_slabs" LAMB's finish launch. "wall" is the time of a whole entry point between two stream
events over a block of calls: it adds the launch gaps and the refresh of the transposed compute copies both entry points end
with. The legs ALTERNATE in blocks of --steps calls after --warmup calls of each, --reps blocks per leg; the yardstick is the
AdamW leg of the same run, and the spread printed is the range of one leg's block means.
   python tools/lamb_bench.py [--reps 7] [--steps 50] [--warmup 10] [--tokens 0,64000] [--out profiles/lamb_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(num_tokens, a, say):
    import numpy as np
    import torch
    import plbert_amd
    from plbert_amd import _lib
    from plbert_amd.engine import HipEngine
    from plbert_amd.train import name_param_groups

    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  num_hidden_layers=12, max_position_embeddings=512)
    eng = HipEngine(cfg, 188, num_tokens, max_batch=2, max_seq=32)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(cfg, 188, num_tokens, seed=0))
    eng._bind()
    eng.sync_weights()
    if num_tokens:   # the token head is stepped only while the last loss call was a dual-head one
        labels, masked, lengths, idx = plbert_amd.synthetic_batch(2, 32, seed=1)
        off, flat = plbert_amd.masked_indices_to_csr(idx)
        dev = lambda x, dt: torch.as_tensor(np.asarray(x), dtype=dt).cuda()
        tok = np.random.RandomState(2).randint(0, num_tokens, size=(2, 32))
        eng.loss_fwd_bwd(dev(masked, torch.int64), dev(labels, torch.int64), None, dev(off, torch.int32), dev(flat, torch.int32),
                         int(off[-1]), token_ids=dev(tok, torch.int64))
    gen = torch.Generator(device="cuda").manual_seed(5)
    eng.grads.copy_(torch.randn(eng.total, device="cuda", generator=gen) * 1e-3)
    hyper = dict(lr=7e-5, betas=(0.9, 0.999), eps=1e-8)
    named = name_param_groups(eng.layout, 0.01, ("bias", "LayerNorm"), ())
    groups = [{**hyper, "weight_decay": g["weight_decay"], "adapt": g["weight_decay"] != 0.0} for g in named]
    group_of = {k: i for i, g in enumerate(named) for k in g["names"]}
    step = [0]

    def nxt():
        step[0] += 1
        return step[0]

    legs = {"adamw": lambda: eng.adamw_step_groups(nxt(), groups, group_of),
            "lamb": lambda: eng.lamb_step(nxt(), groups, group_of)}
    plan = eng.lamb_plan(1, groups, group_of)
    stepped = sum(t["end"] - t["begin"] for t in plan)
    say(f"lamb_bench: {num_tokens} tokens, {stepped} stepped floats in {len(plan)} tensors "
        f"({len(eng.adamw_plan(1, groups, group_of))} AdamW segments); {a.reps} blocks x {a.steps} calls per leg, alternating")
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    kern = {k: {"adamw": [], "reduce_slabs": []} for k in legs}
    wall = {k: [] for k in legs}
    _lib.profile_enable(True)
    try:
        for _ in range(a.reps):
            for name, fn in legs.items():
                _lib.profile_read()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.steps):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                r = _lib.profile_read()
                for cls in kern[name]:
                    kern[name][cls].append(1e3 * r.get(cls, {"ms": 0.0})["ms"] / a.steps)   # us of that class per call
                wall[name].append(1e3 * t0.elapsed_time(t1) / a.steps)
    finally:
        _lib.profile_enable(False)
    total = {}
    for name in legs:
        both = [x + y for x, y in zip(kern[name]["adamw"], kern[name]["reduce_slabs"])]
        total[name] = statistics.median(both)
        say(f"  {name:6s} kernels {total[name]:9.2f} us per call (block means {min(both):.2f} .. {max(both):.2f}; passes "
            f"{statistics.median(kern[name]['adamw']):.2f}, finish {statistics.median(kern[name]['reduce_slabs']):.2f}); "
            f"wall {statistics.median(wall[name]):9.2f} us per call (block means {min(wall[name]):.2f} .. {max(wall[name]):.2f})")
    say(f"  lamb / adamw = {total['lamb'] / total['adamw']:.3f} (kernels), "
        f"{statistics.median(wall['lamb']) / statistics.median(wall['adamw']):.3f} (wall); "
        f"{stepped * 30 / total['adamw'] / 1e6:.2f} TB/s AdamW at 30 B per float, {stepped * 42 / total['lamb'] / 1e6:.2f} TB/s LAMB at 42")
    del eng
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tokens", default="0,64000", help="token-head sizes to measure, comma separated (0: no token head)")
    ap.add_argument("--out", default=None, help="append the summary to this file")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("lamb_bench needs the GPU: a timing taken anywhere else says nothing")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for nt in (int(x) for x in a.tokens.split(",")):
        run(nt, a, say)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
