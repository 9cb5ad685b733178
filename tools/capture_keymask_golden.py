"""Capture tests/golden/keymask_h128.npz: last_hidden_state of transformers.AlbertModel (eager attention, fp32, CPU) under
attention masks that are no prefix — the semantic reference of the key-mask calls (include/plbert.h: plb_*_masked).
   python tools/capture_keymask_golden.py [out.npz]
Tiny model: H 128, 2 heads, E 64, I 128, L 2; B 2, S 40; weights = plbert_amd.deterministic_state_dict(seed, scale) — the
fixture holds the seed, not the weights. Masks: a left pad (13 and 1 positions) and holes (key 0 and a run in sample 0, single
keys and a shorter extent in sample 1). tests/test_keymask_host.py holds oracle.albert_np.encoder_forward to it.
Needs transformers (any version with AlbertModel and attn_implementation="eager"); run once, commit the file."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plbert_amd  # noqa: E402

SEED, SCALE, VOCAB, NPOS, B, S = 41, 0.08, 188, 64, 2, 40
SHAPE = dict(embedding_size=64, hidden_size=128, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
             max_position_embeddings=NPOS, type_vocab_size=2)


def main():
    import transformers
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "keymask_h128.npz")
    pcfg = plbert_amd.AlbertConfig(vocab_size=VOCAB, **SHAPE)
    sd = plbert_amd.deterministic_state_dict(pcfg, VOCAB, seed=SEED, scale=SCALE)
    hcfg = transformers.AlbertConfig(vocab_size=VOCAB, hidden_act="gelu_new", hidden_dropout_prob=0.0,
                                     attention_probs_dropout_prob=0.0, classifier_dropout_prob=0.0, num_hidden_groups=1,
                                     inner_group_num=1, layer_norm_eps=1e-12, attn_implementation="eager", **SHAPE)
    model = transformers.AlbertModel(hcfg).eval()
    own = model.state_dict()
    new = {k[len("encoder."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith("encoder.")}
    missing = [k for k in own if k not in new and not k.endswith("position_ids") and not k.endswith("token_type_ids")]
    assert not missing, missing
    model.load_state_dict(new, strict=False)
    for k, v in model.state_dict().items():
        if k in new:
            assert torch.equal(v, new[k]), k
    rs = np.random.RandomState(SEED)
    ids = rs.randint(1, VOCAB - 2, size=(B, S)).astype(np.int64)
    leftpad = np.ones((B, S), np.int32)
    leftpad[0, :13] = 0
    leftpad[1, :1] = 0
    holes = np.ones((B, S), np.int32)
    holes[0, 0] = 0
    holes[0, 17:23] = 0
    holes[1, [5, 31]] = 0
    holes[1, 33:] = 0          # extent 33 (key 32 is valid)
    res = dict(ids=ids, mask_leftpad=leftpad, mask_holes=holes, seed=np.int64(SEED), scale=np.float64(SCALE),
               vocab_size=np.int64(VOCAB), max_position_embeddings=np.int64(NPOS),
               transformers_version=np.array(transformers.__version__))
    with torch.no_grad():
        for name, m in (("leftpad", leftpad), ("holes", holes)):
            h = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(m)).last_hidden_state
            res["hidden_" + name] = h.numpy().astype(np.float32)
    np.savez_compressed(out, **res)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
