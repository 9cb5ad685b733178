"""token_type_ids / position_ids / inputs_embeds through the Python API (-m gpu): ``AlbertModel.forward`` takes transformers'
arguments with transformers' rules, in inference against a transformers AlbertModel with the same state dict, and on the
``finetune=True`` path with gradients against the float64 reference of tests/embed_inputs_ref.py."""
import numpy as np
import pytest
import torch

import embed_inputs_ref as ref
import plbert_amd
from gpu_util import rel_l2
from oracle import albert_np as onp
from plbert_amd.model import AlbertModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, S, LENS = 3, 40, [40, 33, 7]
SHAPE = dict(embedding_size=64, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2,
             max_position_embeddings=64, type_vocab_size=3)
SETS = {"types": (True, False, False), "positions": (False, True, False), "embeds": (False, False, True),
        "all": (True, True, True)}


def _fixture(**kw):
    pcfg = plbert_amd.AlbertConfig(vocab_size=188, **SHAPE)
    sd = plbert_amd.deterministic_state_dict(pcfg, 188, seed=17)
    rs = np.random.RandomState(5)
    ids = np.zeros((B, S), np.int64)
    for b, n in enumerate(LENS):
        ids[b, :n] = rs.randint(1, 186, size=n)
    bert = AlbertModel(pcfg, max_batch=B, max_seq=S, **kw)
    bert.engine.load_state_dict({k: v for k, v in sd.items() if k.startswith("encoder.")}, strict=False)
    mask = (torch.arange(S)[None, :] < torch.tensor(LENS)[:, None]).int()
    tt, pid, xe = ref.inputs(B, S, LENS, SHAPE["type_vocab_size"], SHAPE["max_position_embeddings"], SHAPE["embedding_size"], 9)
    return bert, sd, ids, mask, tt, pid, xe


def _kw(which, ids, tt, pid, xe, dev):
    use_tt, use_pid, use_xe = SETS[which]
    t = lambda a: torch.as_tensor(a).to(dev)
    return dict(input_ids=None if use_xe else t(ids), token_type_ids=t(tt) if use_tt else None,
                position_ids=t(pid) if use_pid else None, inputs_embeds=t(xe) if use_xe else None)


@pytest.mark.parametrize("which", sorted(SETS))
def test_inference_against_transformers(which):
    """Valid positions within the tolerance tests/test_gpu_model_api.py uses for last_hidden_state: 6e-2 absolute."""
    transformers = pytest.importorskip("transformers")
    bert, sd, ids, mask, tt, pid, xe = _fixture()
    hcfg = transformers.AlbertConfig(vocab_size=188, hidden_act="gelu_new", hidden_dropout_prob=0.0,
                                     attention_probs_dropout_prob=0.0, classifier_dropout_prob=0.0, layer_norm_eps=1e-12,
                                     num_hidden_groups=1, inner_group_num=1, **SHAPE)
    hf = transformers.AlbertModel(hcfg).eval()
    missing, unexpected = hf.load_state_dict({k[len("encoder."):]: torch.as_tensor(np.asarray(v)) for k, v in sd.items()
                                              if k.startswith("encoder.")}, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    with torch.no_grad():
        want = hf(attention_mask=mask, **_kw(which, ids, tt, pid, xe, "cpu")).last_hidden_state.numpy()
        out = bert(attention_mask=mask.to(DEV), **_kw(which, ids, tt, pid, xe, DEV))
    v = (mask != 0).numpy()
    err = np.abs(out.last_hidden_state.cpu().numpy()[v] - want[v]).max()
    print(f"{which}: largest error at a valid position {err:.3e}")
    assert err < 6e-2
    assert tuple(out.pooler_output.shape) == (B, SHAPE["hidden_size"])


@pytest.mark.parametrize("which", ["all", "types"])
def test_finetune_gradients_against_the_reference(which):
    """loss = sum(last_hidden_state * dh): the upstream gradient is dh. Per tensor relative L2 4e-2, the rule of
    tests/test_gpu_encode.py::test_encode_bwd_gradients_against_the_oracle."""
    bert, sd, ids, mask, tt, pid, xe = _fixture(finetune=True)
    v = (mask != 0).numpy()
    dh = np.random.RandomState(3).randn(B, S, SHAPE["hidden_size"]) * 1e-2 * v[..., None]
    kw = _kw(which, ids, tt, pid, xe, DEV)
    embeds = kw["inputs_embeds"] is not None
    if embeds:
        kw["inputs_embeds"].requires_grad_()
    out = bert(attention_mask=mask.to(DEV), **kw)
    assert out.last_hidden_state.requires_grad
    (out.last_hidden_state * torch.as_tensor(dh, dtype=torch.float32).to(DEV)).sum().backward()
    r = {k: (None if x is None else x.cpu().numpy()) for k, x in _kw(which, ids, tt, pid, xe, "cpu").items()}
    _, G, d_sum = ref.reference(onp.Config(**SHAPE), sd, LENS, dh, ids=r["input_ids"], token_type_ids=r["token_type_ids"],
                                position_ids=r["position_ids"],
                                inputs_embeds=None if r["inputs_embeds"] is None else r["inputs_embeds"].astype(np.float64))
    emb = bert.embeddings
    worst = {"type": rel_l2(emb.token_type_embeddings.weight.grad.cpu(), torch.as_tensor(G[ref.TYPE])),
             "position": rel_l2(emb.position_embeddings.weight.grad.cpu(), torch.as_tensor(G[ref.POS]))}
    if embeds:
        assert emb.word_embeddings.weight.grad is None
        worst["inputs_embeds"] = rel_l2(kw["inputs_embeds"].grad.cpu()[torch.as_tensor(v)], torch.as_tensor(d_sum[v]))
        assert not bool(kw["inputs_embeds"].grad.cpu()[torch.as_tensor(~v)].any())
    else:
        worst["word"] = rel_l2(emb.word_embeddings.weight.grad.cpu(), torch.as_tensor(G[ref.WORD]))
    print({k: f"{x:.3e}" for k, x in worst.items()})
    assert all(x < 4e-2 for x in worst.values()), worst
    assert float(emb.token_type_embeddings.weight.grad[1:].abs().max()) > 0      # rows a plain call cannot train
    assert bert.pooler.weight.grad is None


def test_argument_handling():
    bert, sd, ids, mask, tt, pid, xe = _fixture()
    t = lambda a: torch.as_tensor(a).to(DEV)
    am = mask.to(DEV)
    with torch.no_grad():
        # [1,S] position ids are broadcast
        row = np.random.RandomState(1).permutation(SHAPE["max_position_embeddings"])[:S][None, :]
        a = bert(t(ids), attention_mask=am, position_ids=t(row)).last_hidden_state
        b = bert(t(ids), attention_mask=am, position_ids=t(np.tile(row, (B, 1)))).last_hidden_state
        assert torch.equal(a, b)
        plain = bert(t(ids), attention_mask=am).last_hidden_state
        assert not torch.equal(a, plain)
        # the defaults passed explicitly give the plain call's values
        c = bert(t(ids), attention_mask=am, token_type_ids=t(np.zeros((B, S), np.int64)),
                 position_ids=t(np.arange(S)[None, :])).last_hidden_state
        v = am != 0
        assert torch.equal(c[v], plain[v])
        with pytest.raises(ValueError, match="exactly one of input_ids or inputs_embeds"):
            bert(t(ids), attention_mask=am, inputs_embeds=t(xe))
        with pytest.raises(ValueError, match="exactly one of input_ids or inputs_embeds"):
            bert(attention_mask=am, token_type_ids=t(tt))
        bad = tt.copy()
        bad[1, 2] = SHAPE["type_vocab_size"]
        with pytest.raises(ValueError, match=r"token_type_ids.*type_vocab_size = 3"):
            bert(t(ids), attention_mask=am, token_type_ids=t(bad))
        bad = pid.copy()
        bad[0, 0] = SHAPE["max_position_embeddings"]
        with pytest.raises(ValueError, match=r"position_ids.*max_position_embeddings = 64"):
            bert(t(ids), attention_mask=am, position_ids=t(bad))
        bad[0, 0] = -1
        with pytest.raises(ValueError, match="position_ids"):
            bert(t(ids), attention_mask=am, position_ids=t(bad))
        with pytest.raises(ValueError, match="embedding_size"):
            bert(attention_mask=am, inputs_embeds=torch.zeros(B, S, SHAPE["hidden_size"], device=DEV))
