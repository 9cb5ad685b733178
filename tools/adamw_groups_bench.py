"""The grouped AdamW step against plb_adamw_step at full size, on ONE box in ONE process (a tool, not a test; bench.py
measures the whole pre-training step). Config A (768 / 12 heads / FFN 2048, 188 phonemes): 5.85 M stepped floats, 30 B each.
  plain   : plb_adamw_step                          (adamw_kernel: one set of scalars for the range)
  groups  : plb_adamw_step_groups, two-group recipe (no weight decay on names holding "bias" or "LayerNorm")
  frozen  : the same with the three embedding tables frozen (their workgroups leave at the table walk)
  norm    : plb_grad_norm            | norm_groups : plb_grad_norm_groups with the position table frozen
Kernel time comes from the library's own per-launch device events (plb_profile_*, class "adamw" / "reduce_slabs"); the engine's
capacity is tiny (2 x 32) because the optimizer touches parameters only. The legs ALTERNATE in blocks of --steps calls after
--warmup calls of each, --reps blocks per leg; the spread printed is the range of one leg's block means, i.e. what the same
code does from block to block on this box. The grouped launch reads and writes the same bytes as the plain one: a difference
beyond the plain leg's own spread is table-walk overhead.
   python tools/adamw_groups_bench.py [--reps 7] [--steps 50] [--warmup 10] [--out profiles/adamw_groups_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="append the summary to this file")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import plbert_amd
    from plbert_amd import _lib
    from plbert_amd.engine import HipEngine
    from plbert_amd.train import name_param_groups

    if not torch.cuda.is_available():
        raise SystemExit("adamw_groups_bench needs the GPU: a timing taken anywhere else says nothing")
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  num_hidden_layers=12, max_position_embeddings=512)
    eng = HipEngine(cfg, 188, 0, max_batch=2, max_seq=32)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(cfg, 188, seed=0))
    eng._bind()
    eng.sync_weights()
    n = eng.trainable
    gen = torch.Generator(device="cuda").manual_seed(5)
    eng.grads[:n].copy_(torch.randn(n, device="cuda", generator=gen) * 1e-3)
    hyper = dict(lr=7e-5, betas=(0.9, 0.999), eps=1e-8)

    def groups_of(frozen):
        named = name_param_groups(eng.layout, 0.01, ("bias", "LayerNorm"), frozen)
        return [{**hyper, "weight_decay": g["weight_decay"]} for g in named], {k: i for i, g in enumerate(named) for k in g["names"]}

    two, two_of = groups_of(())
    frz, frz_of = groups_of(("embeddings.word", "embeddings.position", "embeddings.token_type"))
    pos_of = {k: 0 for k in eng.layout if "position_embeddings" not in k}
    step = [0]

    def nxt():
        step[0] += 1
        return step[0]

    legs = {
        "plain": ("adamw", lambda: eng.adamw_step(nxt(), weight_decay=0.01, **hyper)),
        "groups": ("adamw", lambda: eng.adamw_step_groups(nxt(), two, two_of)),
        "frozen": ("adamw", lambda: eng.adamw_step_groups(nxt(), frz, frz_of)),
        "norm": ("reduce_slabs", lambda: eng.grad_norm(1.0, 1.0)),
        "norm_groups": ("reduce_slabs", lambda: eng.grad_norm(1.0, 1.0, group_of=pos_of)),
    }
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"adamw_groups_bench: {n} stepped floats, segments: groups {len(eng.adamw_plan(1, two, two_of))}, "
        f"frozen {len(eng.adamw_plan(1, frz, frz_of))}; {a.reps} blocks x {a.steps} calls per leg, alternating")
    for cls, fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    med = {k: [] for k in legs}
    _lib.profile_enable(True)
    try:
        for _ in range(a.reps):
            for name, (cls, fn) in legs.items():
                _lib.profile_read()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                r = _lib.profile_read()[cls]
                med[name].append(1e3 * r["ms"] / a.steps)   # us of that class per call, mean of the block
    finally:
        _lib.profile_enable(False)
    for name, v in med.items():
        say(f"  {name:12s} {statistics.median(v):8.2f} us per call (class '{legs[name][0]}'; block means "
            f"{min(v):.2f} .. {max(v):.2f}, spread {max(v) - min(v):.2f})")
    base, spread = statistics.median(med["plain"]), max(med["plain"]) - min(med["plain"])
    say(f"  groups - plain = {statistics.median(med['groups']) - base:+.2f} us against the plain leg's spread of {spread:.2f} us")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
