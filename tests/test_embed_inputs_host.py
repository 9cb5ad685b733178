"""Embedding inputs (token_type_ids / position_ids / inputs_embeds), host side (no GPU): the reference the GPU tests use
(tests/embed_inputs_ref.py: the oracle driven through a synthetic word table) is held to transformers' AlbertModel in
float64, and the ctypes mirrors of the two new structs have the compiler's layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import c_header
import embed_inputs_ref as ref
import plbert_amd
from oracle import albert_np as onp
from plbert_amd import _lib
from test_binding_host import ROCM, _compiler

B, S, LENS = 3, 24, [24, 17, 5]
CFG = dict(embedding_size=16, hidden_size=128, num_attention_heads=2, intermediate_size=64, num_hidden_layers=2,
           max_position_embeddings=40, type_vocab_size=3)


def _model():
    transformers = pytest.importorskip("transformers")
    pcfg = plbert_amd.AlbertConfig(vocab_size=50, **CFG)
    sd = {k: np.asarray(v, np.float64) for k, v in plbert_amd.deterministic_state_dict(pcfg, 8, seed=5).items()}
    rs = np.random.RandomState(3)
    for k in (ref.WORD, ref.POS, ref.TYPE):   # every row of every table distinct and of a size that shows
        sd[k] = rs.randn(*sd[k].shape)
    hcfg = transformers.AlbertConfig(vocab_size=50, hidden_act="gelu_new", hidden_dropout_prob=0.0,
                                     attention_probs_dropout_prob=0.0, classifier_dropout_prob=0.0, layer_norm_eps=1e-12,
                                     num_hidden_groups=1, inner_group_num=1, **CFG)
    hf = transformers.AlbertModel(hcfg).double().train()
    missing, unexpected = hf.load_state_dict({k[len("encoder."):]: torch.from_numpy(v) for k, v in sd.items()
                                              if k.startswith("encoder.")}, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return onp.Config(vocab_size=50, **CFG), sd, hf


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
    print(f"{what}: max error relative to the tensor's largest element {err:.3e}")
    assert err < 1e-9, (what, err)


@pytest.mark.parametrize("embeds", [False, True])
def test_the_reference_agrees_with_transformers(embeds):
    ocfg, sd, hf = _model()
    rs = np.random.RandomState(11)
    ids = np.zeros((B, S), np.int64)
    for b, n in enumerate(LENS):
        ids[b, :n] = rs.randint(1, 50, size=n)
    tt, pid, xe = ref.inputs(B, S, LENS, CFG["type_vocab_size"], CFG["max_position_embeddings"], CFG["embedding_size"], 7)
    valid = np.arange(S)[None, :] < np.asarray(LENS)[:, None]
    dh = rs.randn(B, S, CFG["hidden_size"]) * valid[..., None]
    hidden, G, d_sum = ref.reference(ocfg, sd, LENS, dh, ids=None if embeds else ids, token_type_ids=tt, position_ids=pid,
                                     inputs_embeds=xe.astype(np.float64) if embeds else None)
    x = torch.from_numpy(xe.astype(np.float64)).requires_grad_() if embeds else None
    out = hf(input_ids=None if embeds else torch.from_numpy(ids), attention_mask=torch.from_numpy(valid.astype(np.int64)),
             token_type_ids=torch.from_numpy(tt), position_ids=torch.from_numpy(pid), inputs_embeds=x).last_hidden_state
    _close(out.detach().numpy()[valid], hidden[valid], "hidden")
    out.backward(torch.from_numpy(dh))
    grads = {"encoder." + n: p.grad for n, p in hf.named_parameters()}
    assert len(G) == len([n for n in grads if "pooler" not in n])
    for name, want in G.items():
        if embeds and name == ref.WORD:
            assert grads[name] is None and not want.any()
            continue
        if name.endswith("attention.key.bias"):   # true gradient 0 (softmax is shift invariant): both are rounding noise,
            scale = np.abs(G[name.replace("key", "query")]).max()   # measured against the query bias's gradient
            assert max(np.abs(want).max(), grads[name].abs().max().item()) < 1e-9 * scale, name
            continue
        _close(want, grads[name].numpy(), name)
    if embeds:
        _close(d_sum, x.grad.numpy(), "inputs_embeds.grad")
    assert G[ref.TYPE][1:].any() and not G[ref.WORD][0].any()


def test_new_struct_mirrors_have_the_compilers_layout(tmp_path):
    hdrs = {"PlbEmbedInputs": c_header.public(), "PlbEmbedIn": c_header.kernels()}
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "plbert_kernels.h"', '#include "plbert.h"', "int main() {"]
    for name, hdr in hdrs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for f in hdr.structs[name]:
            lines.append(f'  printf("{name}.{f.name} %zu %zu\\n", offsetof({name}, {f.name}), sizeof((({name}*)0)->{f.name}));')
    lines += ["  return 0;", "}", ""]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines))
    cmd = [_compiler(), "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", "-I",
           os.path.join(c_header.ROOT, "plbert_amd", "csrc"), "-I", os.path.join(c_header.ROOT, "include"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    want = {}
    for ln in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines():
        what, *nums = ln.split()
        want[what] = tuple(int(n) for n in nums)
    for name in hdrs:
        cls = getattr(_lib, name)
        assert C.sizeof(cls) == want[name][0], name
        assert [f[0] for f in cls._fields_] == [f.name for f in hdrs[name].structs[name]]
        for fname, ftype in cls._fields_:
            assert (getattr(cls, fname).offset, getattr(cls, fname).size) == want[f"{name}.{fname}"], (name, fname)
    assert [f[0] for f in _lib.PlbEmbedInputs._fields_] == ["token_type_ids", "position_ids", "inputs_embeds"]
    assert _lib.PlbEmbedIn._fields_[0] == ("base", C.c_void_p)


def test_the_entry_points_are_exported_and_bound():
    L = _lib.lib()
    hdr = c_header.public()
    for name in ("plb_forward_inputs", "plb_encode_inputs", "plb_encode_bwd_inputs"):
        assert hasattr(L, name) and name in _lib.PUBLIC
        texts = c_header.c_params(hdr, name)
        assert texts[:3] == ["PlbEngine* e", "const int64_t* ids", "const PlbEmbedInputs* inputs"] and texts[-1] == "void* stream"
    assert c_header.c_params(hdr, "plb_encode_bwd_inputs")[-2] == "float* d_inputs_embeds"
    assert "embed_inputs.hip" in __import__("plbert_amd.build", fromlist=["SOURCES"]).SOURCES
    # 512-token chunks: one [P + type rows][E] block of partial rows per chunk
    assert L.plb_embed_inputs_part_floats(512, 512, 2, 128) == 514 * 128
    assert L.plb_embed_inputs_part_floats(513, 512, 2, 128) == 2 * 514 * 128
    assert L.plb_embed_inputs_part_floats(0, 512, 2, 128) == 0
