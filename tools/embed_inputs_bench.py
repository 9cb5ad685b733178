"""What the embedding inputs cost on top of a differentiable forward + backward: python tools/embed_inputs_bench.py [--rounds 9]

 plain    plb_encode + plb_encode_bwd (ids alone: the launches of embed.hip);
 inputs   plb_encode_inputs + plb_encode_bwd_inputs with token_type_ids, position_ids, inputs_embeds and d_inputs_embeds
          (embed_inputs.hip: the row kernel with per-token sources, the keyed table sums in 512-token chunks, the unpacked
          gradient of the pre-LayerNorm sum).

Shape: 32 x 512, hidden 768, 12 heads, 12 applications (config A), type_vocab_size 2, no padding. The two pairs are warmed,
then run alternately in one process; every timed pair ends with a device synchronise (wall time between two synchronises).
A second pass of alternating pairs runs with the engine's profiler on and reports, per pair, the time and the launch
count of the embedding classes (plb_profile_read) — the rest of a pair is the same launches in both. Prints the medians, the
per-class figures and one JSON line; --out also writes the text to a file (profiles/embed_inputs_ab.txt)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plbert_amd  # noqa: E402
from plbert_amd import _lib  # noqa: E402
from plbert_amd.engine import HipEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, S, nl = a.batch, a.seq, a.layers
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  max_position_embeddings=512, num_hidden_layers=nl)
    H, E = cfg.hidden_size, cfg.embedding_size
    eng = HipEngine(cfg, 188, 0, max_batch=B, max_seq=S)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(cfg, 188, 0, seed=3))
    rng = np.random.default_rng(0)
    dev = eng.device
    ids = torch.from_numpy(rng.integers(1, 185, size=(B, S)).astype(np.int64)).to(dev)
    tt = torch.from_numpy(rng.integers(0, cfg.type_vocab_size, size=(B, S)).astype(np.int64)).to(dev)
    pid = torch.from_numpy(rng.integers(0, cfg.max_position_embeddings, size=(B, S)).astype(np.int64)).to(dev)
    xe = torch.from_numpy(rng.standard_normal((B, S, E)).astype(np.float32)).to(dev)
    dh = torch.from_numpy((rng.standard_normal((B, S, H)) * 1e-2).astype(np.float32)).to(dev)

    def plain():
        eng.encode(ids)
        eng.encode_bwd(dh)

    def inputs():
        eng.encode(None, token_type_ids=tt, position_ids=pid, inputs_embeds=xe)
        eng.encode_bwd(dh, want_d_inputs_embeds=True)

    paths = {"plain": plain, "inputs": inputs}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):                                            # warm: workspace, kernels
        for fn in paths.values():
            timed(fn)
    times = {k: [] for k in paths}
    for _ in range(a.rounds):                                     # alternated
        for k, fn in paths.items():
            times[k].append(timed(fn))
    # per-class figures of the same alternation, profiler on (every launch bracketed by events: the pair itself is slower)
    _lib.profile_enable(True)
    _lib.profile_read()
    prof = {k: {} for k in paths}
    for _ in range(a.rounds):
        for k, fn in paths.items():
            fn()
            torch.cuda.synchronize()
            for cls, v in _lib.profile_read().items():
                c = prof[k].setdefault(cls, dict(ms=[], launches=v["launches"]))
                c["ms"].append(v["ms"])
                assert c["launches"] == v["launches"], (k, cls)
    _lib.profile_enable(False)
    res = {"shape": [B, S, H, E], "layers": nl, "rounds": a.rounds}
    lines = []
    for k in paths:
        res[f"{k}_ms_median"] = round(statistics.median(times[k]), 3)
        res[f"{k}_ms_min"] = round(min(times[k]), 3)
        lines.append(f"{k:7s} pair (encode + encode_bwd): median {res[k + '_ms_median']} ms, min {res[k + '_ms_min']} ms")
    res["delta_ms_median"] = round(res["inputs_ms_median"] - res["plain_ms_median"], 3)
    lines.append(f"inputs - plain: {res['delta_ms_median']} ms per pair ({100 * res['delta_ms_median'] / res['plain_ms_median']:.2f} %)")
    lines.append("per class and pair (profiler on; median ms, launches):   plain | inputs")
    res["classes"] = {}
    for cls in sorted(set(prof["plain"]) | set(prof["inputs"])):
        row = {}
        for k in paths:
            c = prof[k].get(cls)
            row[k] = None if c is None else [round(statistics.median(c["ms"]), 4), c["launches"]]
        res["classes"][cls] = row
        emb = "embed" in cls.lower()
        if emb or row["plain"] is None or row["inputs"] is None or row["plain"][1] != row["inputs"][1]:
            lines.append(f"  {cls:24s} {row['plain']} | {row['inputs']}")
    same = [c for c, r in res["classes"].items() if r["plain"] and r["inputs"] and r["plain"][1] == r["inputs"][1]]
    lines.append(f"  ({len(same)} of {len(res['classes'])} classes have the same launch count in both pairs)")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
