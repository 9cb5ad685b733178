"""Fine-tuning through the Python API (-m gpu): ``AlbertModel(cfg, finetune=True)`` inside a downstream torch model, as the
reference README's "Finetuning" section uses a PL-BERT checkpoint — ``bert(texts, attention_mask=...).last_hidden_state``
feeds the caller's layers, ``loss.backward()`` reaches the encoder through plb_encode_bwd, torch's or this library's AdamW
steps it. On the small_h128 fixture's config, weights and batch (B = 3, S = 40, lengths 40 / 33 / 7)."""
import numpy as np
import pytest
import torch
from torch import nn

from conftest import golden_cfg, load_golden
import plbert_amd
from plbert_amd.model import AlbertModel, PhonemeOnlyModel
from plbert_amd.train import AdamW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fixture():
    g = load_golden("small_h128")
    _, pcfg, sd = golden_cfg(g)
    ids = torch.as_tensor(np.asarray(g["masked"])).to(DEV)
    lens = torch.as_tensor(np.asarray(g["lengths"], np.int64)).to(DEV)
    mask = (torch.arange(ids.shape[1], device=DEV)[None, :] < lens[:, None]).int()
    return g, pcfg, sd, ids, mask


def _bert(pcfg, sd, ids, **kw):
    bert = AlbertModel(pcfg, max_batch=ids.shape[0], max_seq=ids.shape[1], **kw)
    bert.engine.load_state_dict({k: v for k, v in sd.items() if k.startswith("encoder.")}, strict=False)
    return bert


def _downstream(H, seed=0):
    torch.manual_seed(seed)
    lin = nn.Linear(H, 64).to(DEV)
    target = torch.randn(3, 40, 64, device=DEV)
    return lin, target


def _loss(bert, lin, target, ids, mask):
    out = bert(ids, attention_mask=mask)
    return ((lin(out.last_hidden_state) - target) ** 2 * mask[..., None]).mean(), out


def test_backward_reaches_every_encoder_parameter():
    g, pcfg, sd, ids, mask = _fixture()
    bert = _bert(pcfg, sd, ids, finetune=True)
    assert bert.differentiable and bert.engine.train_mode
    lin, target = _downstream(pcfg.hidden_size)
    loss, out = _loss(bert, lin, target, ids, mask)
    assert out.last_hidden_state.requires_grad and not out.pooler_output.requires_grad
    assert float(out.last_hidden_state[mask == 0].abs().max()) == 0.0          # zeros at the pad positions
    loss.backward()
    eng = bert.engine
    seen = 0
    for n, p in bert.named_parameters():
        if n.startswith("pooler."):
            assert p.grad is None
            continue
        off, size, shp = eng.layout["encoder." + n]
        assert p.grad is not None and torch.equal(p.grad, eng.grads[off:off + size].view(shp)), n
        assert float(p.grad.abs().max()) > 0 or "key.bias" in n or "word_embeddings" in n, n
        seen += 1
    assert seen == 23
    assert lin.weight.grad is not None and float(lin.weight.grad.abs().max()) > 0 and lin.bias.grad is not None
    # under no_grad / in eval mode the forward is the plain one
    with torch.no_grad():
        assert not bert(ids, attention_mask=mask).last_hidden_state.requires_grad
    bert.eval()
    assert not bert(ids, attention_mask=mask).last_hidden_state.requires_grad


@pytest.mark.parametrize("which", ["torch", "plbert"])
def test_fifteen_finetuning_steps_lower_the_loss(which):
    g, pcfg, sd, ids, mask = _fixture()
    bert = _bert(pcfg, sd, ids, finetune=True)
    lin, target = _downstream(pcfg.hidden_size)
    if which == "torch":   # the reference README's step 2: torch.optim.AdamW over the views of the flat buffer
        opts = [torch.optim.AdamW(list(bert.parameters()) + list(lin.parameters()), lr=1e-3)]
    else:
        opts = [AdamW(bert.parameters(), lr=1e-3, model=bert), torch.optim.AdamW(lin.parameters(), lr=1e-3)]
    p0 = bert.engine.params.clone()
    losses = []
    for _ in range(15):
        for o in opts:
            o.zero_grad()
        loss, _ = _loss(bert, lin, target, ids, mask)
        loss.backward()
        for o in opts:
            o.step()
        losses.append(float(loss.item()))
        assert bert.engine.poll_status()["ln_exchange_timeouts"] == 0   # (a torch optimizer has no device-side skip)
    print(which, "losses", [round(x, 5) for x in losses])
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), losses
    eng = bert.engine
    head0 = eng.layout["phoneme_predictor.weight"][0]
    assert not torch.equal(eng.params[:head0], p0[:head0])
    assert torch.equal(eng.params[head0:], p0[head0:])        # stand-in head and pooler: no gradient, no update


def test_wrapped_encoder_becomes_differentiable_and_gives_the_same_gradients():
    g, pcfg, sd, ids, mask = _fixture()
    lin, target = _downstream(pcfg.hidden_size)
    bert = _bert(pcfg, sd, ids, finetune=True)
    _loss(bert, lin, target, ids, mask)[0].backward()
    head0 = bert.engine.layout["phoneme_predictor.weight"][0]
    want = bert.engine.grads[:head0].clone()
    lin_grad = lin.weight.grad.clone()
    lin.zero_grad()

    model = PhonemeOnlyModel(AlbertModel(pcfg, max_batch=3, max_seq=40), int(g["num_phonemes"]), pcfg.hidden_size)
    model.engine.load_state_dict(sd)
    enc = model.encoder
    assert not enc.differentiable
    assert not enc(ids, attention_mask=mask).last_hidden_state.requires_grad
    enc.differentiable = True
    loss, out = _loss(enc, lin, target, ids, mask)
    assert out.last_hidden_state.requires_grad
    loss.backward()
    assert model.engine.layout["phoneme_predictor.weight"][0] == head0
    assert torch.equal(model.engine.grads[:head0], want) and torch.equal(lin.weight.grad, lin_grad)
    assert model.phoneme_predictor.weight.grad is None


def test_default_model_is_unchanged():
    g, pcfg, sd, ids, mask = _fixture()
    bert = _bert(pcfg, sd, ids)
    assert not bert.differentiable and not bert.engine.train_mode and bert.training and torch.is_grad_enabled()
    out = bert(ids, attention_mask=mask)
    assert not out.last_hidden_state.requires_grad and not out.pooler_output.requires_grad
    lens = mask.sum(1).to(torch.int32)
    hid, _, _ = bert.engine.forward(ids, lens, want_hidden=True, want_phoneme=False)
    assert torch.equal(out.last_hidden_state.view(torch.int32), hid.view(torch.int32))
    bert.differentiable = True   # an inference engine cannot keep the activations: a clear error, no quiet fall-back
    with pytest.raises(RuntimeError, match="train=False"):
        bert(ids, attention_mask=mask)


def test_backward_of_an_overwritten_forward_raises():
    g, pcfg, sd, ids, mask = _fixture()
    bert = _bert(pcfg, sd, ids, finetune=True)
    first = bert(ids, attention_mask=mask).last_hidden_state
    second = bert(ids, attention_mask=mask).last_hidden_state
    with pytest.raises(RuntimeError, match="a later engine call overwrote"):
        first.sum().backward()
    second.sum().backward()                                   # the newer one still has its activations
    third = bert(ids, attention_mask=mask).last_hidden_state
    bert.engine.forward(ids, mask.sum(1).to(torch.int32))     # any computing call ends the life of the stash
    with pytest.raises(RuntimeError, match="a later engine call overwrote"):
        third.sum().backward()


def test_param_groups_lr_changes_the_next_step():
    g, pcfg, sd, ids, mask = _fixture()
    bert = _bert(pcfg, sd, ids, finetune=True)
    lin, target = _downstream(pcfg.hidden_size)
    opt = AdamW(bert.parameters(), lr=1e-3, model=bert)
    for grp in opt.param_groups:
        grp["lr"] = 0.0
    p0 = bert.engine.params.clone()
    _loss(bert, lin, target, ids, mask)[0].backward()
    opt.step()
    assert torch.equal(bert.engine.params, p0)                # lr 0: decay factor 1, step size 0
    opt.param_groups[0]["lr"] = 1e-3
    opt.zero_grad()
    _loss(bert, lin, target, ids, mask)[0].backward()
    opt.step()
    moved = (bert.engine.params - p0).abs().max()
    assert 1e-4 < float(moved) < 1e-2, float(moved)
