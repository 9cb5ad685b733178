"""What the per-application outputs cost on top of a forward: python tools/layer_outputs_bench.py [--rounds 7]

 plain    plb_forward with the hidden output (what AlbertModel.forward runs without the flags);
 hidden   plb_forward_layers with every hidden state (L + 1 conversion passes of B*S*H floats);
 all      plb_forward_layers with every hidden state and every attention map (L launches that write B*NH*S*S floats each:
          403 MB per application at 32 x 12 x 512 x 512).

Shape: 32 x 512, hidden 768, 12 heads, 12 applications (config A), inference-only engine. The outputs are allocated once
and reused (``out=``), so allocator time is not in the figures. The three paths are warmed, then run alternately; every
timed run ends with a device synchronise (wall time between two synchronises). Prints the median and the minimum per
path, the store bandwidth the attention maps reach over the plain forward's time, then one JSON line."""
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
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    B, S, nl = a.batch, a.seq, a.layers
    cfg = plbert_amd.AlbertConfig(vocab_size=188, hidden_size=768, num_attention_heads=12, intermediate_size=2048,
                                  max_position_embeddings=512, num_hidden_layers=nl)
    H, NH = cfg.hidden_size, cfg.num_attention_heads
    eng = HipEngine(cfg, 188, 0, max_batch=B, max_seq=S, train=False)
    eng.load_state_dict(plbert_amd.deterministic_state_dict(cfg, 188, 0, seed=3))
    ids = torch.from_numpy(np.random.default_rng(0).integers(1, 185, size=(B, S)).astype(np.int64)).to(eng.device)
    hs = [torch.empty((B, S, H), dtype=torch.float32, device=eng.device) for _ in range(nl + 1)]
    at = [torch.empty((B, NH, S, S), dtype=torch.float32, device=eng.device) for _ in range(nl)]

    paths = {
        "plain": lambda: eng.forward(ids, None, want_hidden=True, want_phoneme=False),
        "hidden": lambda: eng.forward_layers(ids, None, out=(hs, [None] * nl)),
        "all": lambda: eng.forward_layers(ids, None, out=(hs, at)),
    }

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
    res = {"shape": [B, S, H, NH], "layers": nl}
    for k in paths:
        res[f"{k}_ms_median"] = round(statistics.median(times[k]), 3)
        res[f"{k}_ms_min"] = round(min(times[k]), 3)
    map_bytes = nl * B * NH * S * S * 4
    extra = res["all_ms_median"] - res["hidden_ms_median"]
    res["attention_maps_gb"] = round(map_bytes / 1e9, 3)
    res["attention_maps_tb_per_s"] = round(map_bytes / 1e12 / (extra / 1e3), 3) if extra > 0 else None
    print(f"plain   plb_forward(hidden)                       : median {res['plain_ms_median']} ms, min {res['plain_ms_min']} ms")
    print(f"hidden  plb_forward_layers, {nl + 1} hidden states       : median {res['hidden_ms_median']} ms, min {res['hidden_ms_min']} ms")
    print(f"all     ... and {nl} attention maps ({res['attention_maps_gb']} GB)      : median {res['all_ms_median']} ms, min {res['all_ms_min']} ms"
          f" ({res['attention_maps_tb_per_s']} TB/s of stores over the hidden-states run)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
