"""Token-head predictions, two ways, on one engine in one process: python tools/token_topk_bench.py [--rounds 7]

 A  a forward that outputs nothing + plb_token_report on every position (fused GEMM + top-k, no logits stored);
 B  plb_forward with token_logits (fp32 [B,S,num_tokens]) + torch.topk on it — the only path before plb_token_report.

Shape: 32 x 512, num_tokens 64000, k = 5, hidden 768 (12 layers, inference-only engine). Both paths are warmed, then run
alternately; every timed run ends with a device synchronise (wall time between two synchronises). Prints the median and the
minimum per path, the encoder-only forward for scale, and the peak device memory of each path above the engine's own buffers,
then one JSON line."""
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
from plbert_amd.engine import HipEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--tokens", type=int, default=64000)
    ap.add_argument("--topk", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    B, S, k = a.batch, a.seq, a.topk
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  max_position_embeddings=512, num_hidden_layers=a.layers)
    eng = HipEngine(cfg, 188, a.tokens, max_batch=B, max_seq=S, train=False)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(cfg, 188, a.tokens, seed=3))
    ids = torch.from_numpy(np.random.default_rng(0).integers(1, 185, size=(B, S)).astype(np.int64)).to(eng.device)
    out = {"topk_ids": torch.empty((B * S, k), dtype=torch.int32, device=eng.device),
           "topk_logprob": torch.empty((B * S, k), dtype=torch.float32, device=eng.device)}

    def encoder_only():
        eng.forward(ids, None, want_hidden=False, want_phoneme=False, want_token=False)

    def path_a():
        eng.forward(ids, None, want_hidden=False, want_phoneme=False, want_token=False)
        return eng.token_report(None, None, topk=k, want=("topk_ids", "topk_logprob"), out=out)["topk_ids"]

    def path_b():
        _, _, tk = eng.forward(ids, None, want_hidden=False, want_phoneme=False, want_token=True)
        v, i = torch.topk(tk, k, dim=-1)
        return i

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    for fn in (encoder_only, path_a, path_b, path_a, path_b):     # warm: workspace, allocator, kernels
        timed(fn)
    base = torch.cuda.memory_allocated()
    peaks = {}
    for name, fn in (("A", path_a), ("B", path_b)):
        torch.cuda.reset_peak_memory_stats()
        _, r = timed(fn)
        peaks[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        del r
    times = {"A": [], "B": [], "encoder": []}
    ia = ib = None
    for _ in range(a.rounds):                                     # alternated
        t, ia = timed(path_a)
        times["A"].append(t)
        t, ib = timed(path_b)
        times["B"].append(t)
        t, _ = timed(encoder_only)
        times["encoder"].append(t)
    agree = float((ia.view(B, S, k).to(torch.int64) == ib).float().mean())
    res = {"shape": [B, S, a.tokens, k], "layers": a.layers}
    for name in ("A", "B", "encoder"):
        res[f"{name}_ms_median"] = round(statistics.median(times[name]), 3)
        res[f"{name}_ms_min"] = round(min(times[name]), 3)
    res["A_peak_mib"], res["B_peak_mib"] = round(peaks["A"], 1), round(peaks["B"], 1)
    res["ids_equal_fraction"] = round(agree, 6)
    print(f"A  forward without logits + plb_token_report : median {res['A_ms_median']} ms, min {res['A_ms_min']} ms, peak {res['A_peak_mib']} MiB above the engine")
    print(f"B  plb_forward(token_logits) + torch.topk     : median {res['B_ms_median']} ms, min {res['B_ms_min']} ms, peak {res['B_peak_mib']} MiB above the engine")
    print(f"   encoder-only forward                        : median {res['encoder_ms_median']} ms")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
