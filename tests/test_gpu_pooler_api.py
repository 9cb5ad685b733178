"""A differentiable ``pooler_output`` through the Python API (-m gpu): ``AlbertModel(cfg, finetune=True, train_pooler=True)``
under a sentence-level head, the pattern of AlbertForSequenceClassification. On the small_h128 fixture's config, weights and
batch (B = 3, S = 40, lengths 40 / 33 / 7).

Opt-in on: the output requires grad, a loss on it reaches every encoder parameter and the pooler's two, the pooler's gradients
are the views of ``engine.grads`` and lie within the derived bound (tests/pooler_ref.py) of float64 autograd; a loss on both
outputs composes bit for bit; fifteen steps of either AdamW lower a pooled-output loss; the optimizer state round-trips with
the pooler's moments. Opt-in off (the default): the detached output, the gradients and the launches of a plain encode_bwd."""
import numpy as np
import pytest
import torch
from torch import nn

from conftest import golden_cfg, load_golden
import pooler_ref as R
from pooler_gpu import POOL_B, POOL_W, launcher
from plbert_amd import _lib
from plbert_amd.model import AlbertModel, PhonemeOnlyModel
from plbert_amd.train import AdamW, Lamb

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


def _head(H, seed=0, classes=8):
    torch.manual_seed(seed)
    return nn.Linear(H, classes).to(DEV), torch.randn(3, classes, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_a_loss_on_pooler_output_reaches_the_pooler_and_every_encoder_parameter():
    g, pcfg, sd, ids, mask = _fixture()
    bert = _bert(pcfg, sd, ids, finetune=True, train_pooler=True)
    assert bert.differentiable and bert.train_pooler
    cls, target = _head(pcfg.hidden_size)
    out = bert(ids, attention_mask=mask)
    assert out.pooler_output.requires_grad and out.last_hidden_state.requires_grad
    assert torch.equal(_bits(out.pooler_output), _bits(bert.engine.pooler(out.last_hidden_state.detach())))
    seen = {}
    out.pooler_output.register_hook(lambda gr: seen.setdefault("P", gr.clone()))
    ((cls(out.pooler_output) - target) ** 2).mean().backward()
    eng = bert.engine
    n_enc = 0
    for n, p in bert.named_parameters():
        off, size, shp = eng.layout["encoder." + n]
        assert p.grad is not None and torch.equal(p.grad, eng.grads[off:off + size].view(shp)), n
        assert float(p.grad.abs().max()) > 0 or "key.bias" in n or "word_embeddings" in n, n
        n_enc += not n.startswith("pooler.")
    assert n_enc == 23 and bert.pooler.weight.grad is not None and bert.pooler.bias.grad is not None
    # against float64 autograd over (last_hidden_state[:, 0], W, b), within the derived bound
    h0 = out.last_hidden_state.detach()[:, 0].double().requires_grad_(True)
    W = bert.pooler.weight.detach().double().requires_grad_(True)
    b = bert.pooler.bias.detach().double().requires_grad_(True)
    y64 = torch.tanh(nn.functional.linear(h0, W, b))
    y64.backward(seen["P"].double())
    f = lambda t: t.detach().cpu().numpy()
    y32 = f(out.pooler_output)
    at_y32 = R.backward(f(h0), f(W), f(b), f(seen["P"]), y=y32)
    e_dpre, e_dW, e_db, _ = R.bounds(f(h0), f(W), f(seen["P"]), y32)
    # float64 autograd differentiates at ITS y: the difference of the two restatements (exact in float64, a function of the
    # forward's own error |y32 - y64| alone) joins the bound
    at_y64 = R.backward(f(h0), f(W), f(b), f(seen["P"]))
    assert np.abs(at_y64[1] - f(W.grad)).max() <= 1e-12 and np.abs(at_y64[2] - f(b.grad)).max() <= 1e-12
    for name, got, k, e in (("pooler.weight", bert.pooler.weight.grad, 1, e_dW), ("pooler.bias", bert.pooler.bias.grad, 2, e_db)):
        err32 = np.abs(f(got).astype(np.float64) - at_y32[k])
        err64 = np.abs(f(got).astype(np.float64) - (f(W.grad) if k == 1 else f(b.grad)))
        fwd = np.abs(at_y32[k] - at_y64[k])
        print(f"{name}: max err at the pooler's y {err32.max():.3e} (bound {e.max():.3e}), against float64 autograd "
              f"{err64.max():.3e} (forward share {fwd.max():.3e})")
        assert (err32 <= e).all(), name
        assert (err64 <= e + fwd + 1e-12).all(), name


def test_a_loss_on_both_outputs_composes_bit_for_bit():
    g, pcfg, sd, ids, mask = _fixture()
    bert = _bert(pcfg, sd, ids, finetune=True, train_pooler=True)
    cls, target = _head(pcfg.hidden_size)
    torch.manual_seed(1)
    lin, tgt2 = nn.Linear(pcfg.hidden_size, 16).to(DEV), torch.randn(3, 40, 16, device=DEV)
    out = bert(ids, attention_mask=mask)
    seen = {}
    out.pooler_output.register_hook(lambda gr: seen.setdefault("P", gr.clone()))
    out.last_hidden_state.register_hook(lambda gr: seen.setdefault("G", gr.clone()))
    loss = ((cls(out.pooler_output) - target) ** 2).mean() + ((lin(out.last_hidden_state) - tgt2) ** 2 * mask[..., None]).mean()
    loss.backward()
    eng = bert.engine
    got = eng.grads.clone()
    head0, p0 = eng.layout["phoneme_predictor.weight"][0], eng.layout[POOL_W][0]
    p1 = eng.layout[POOL_B][0] + eng.layout[POOL_B][1]
    lens = mask.sum(1).to(torch.int32)
    hid = eng.encode(ids, lens)
    assert torch.equal(_bits(hid), _bits(out.last_hidden_state.detach()))
    dwb, dh0 = launcher(eng, hid, seen["P"])
    G2 = seen["G"].clone()
    G2[:, 0] = G2[:, 0] + dh0
    eng.encode_bwd(G2)
    assert torch.equal(_bits(eng.grads[:head0]), _bits(got[:head0]))
    assert torch.equal(_bits(got[p0:p1]), _bits(dwb)) and not bool(got[head0:p0].any())


@pytest.mark.parametrize("which", ["torch", "plbert"])
def test_fifteen_steps_lower_a_pooled_output_loss_and_move_the_pooler(which):
    g, pcfg, sd, ids, mask = _fixture()
    bert = _bert(pcfg, sd, ids, finetune=True, train_pooler=True)
    cls, target = _head(pcfg.hidden_size)
    if which == "torch":
        opts = [torch.optim.AdamW(list(bert.parameters()) + list(cls.parameters()), lr=1e-3)]
    else:
        opts = [AdamW(bert.parameters(), lr=1e-3, model=bert), torch.optim.AdamW(cls.parameters(), lr=1e-3)]
    eng = bert.engine
    p_start = eng.params.clone()
    losses = []
    for _ in range(15):
        for o in opts:
            o.zero_grad()
        loss = ((cls(bert(ids, attention_mask=mask).pooler_output) - target) ** 2).mean()
        loss.backward()
        for o in opts:
            o.step()
        losses.append(float(loss.item()))
        assert eng.poll_status()["ln_exchange_timeouts"] == 0
    print(which, "losses", [round(x, 5) for x in losses])
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), losses
    head0, p0 = eng.layout["phoneme_predictor.weight"][0], eng.layout[POOL_W][0]
    nw, nb = eng.layout[POOL_W][1], eng.layout[POOL_B][1]
    assert not torch.equal(eng.params[:head0], p_start[:head0])
    assert not torch.equal(eng.params[p0:p0 + nw], p_start[p0:p0 + nw])                 # pooler.weight moved
    assert not torch.equal(eng.params[p0 + nw:p0 + nw + nb], p_start[p0 + nw:p0 + nw + nb])   # pooler.bias moved
    assert torch.equal(eng.params[head0:p0], p_start[head0:p0])                         # the stand-in head: no gradient, no update
    if which == "plbert":   # the state dict holds the pooler's moments at the shared step count, and round-trips
        names = ["encoder." + n for n, _ in bert.named_parameters()]
        sd_opt = opts[0].state_dict()
        assert set(sd_opt["state"]) == set(range(len(names)))
        for n in (POOL_W, POOL_B):
            st = sd_opt["state"][names.index(n)]
            off, size, shp = eng.layout[n]
            assert float(st["step"]) == 15.0 and float(st["exp_avg_sq"].abs().max()) > 0
            assert torch.equal(st["exp_avg"], eng.exp_avg[off:off + size].view(shp))
        bert2 = _bert(pcfg, sd, ids, finetune=True, train_pooler=True)
        opt2 = AdamW(bert2.parameters(), lr=5.0, model=bert2)
        assert names.index(POOL_W) not in opt2.state_dict()["state"]                    # never stepped: no state
        opt2.load_state_dict(sd_opt)
        again = opt2.state_dict()
        assert opt2.step_count == 15 and set(again["state"]) == set(sd_opt["state"]) and again["param_groups"] == sd_opt["param_groups"]
        for i, st in sd_opt["state"].items():
            assert torch.equal(again["state"][i]["exp_avg"], st["exp_avg"]) and torch.equal(again["state"][i]["exp_avg_sq"], st["exp_avg_sq"])


def test_grouped_optimizers_give_the_pooler_state_once_it_has_been_stepped():
    g, pcfg, sd, ids, mask = _fixture()
    cls, target = _head(pcfg.hidden_size)
    for make in (lambda m: Lamb(m.parameters(), lr=1e-3, model=m), lambda m: AdamW([{"params": list(m.parameters())}], lr=1e-3, model=m)):
        bert = _bert(pcfg, sd, ids, finetune=True, train_pooler=True)
        opt = make(bert)
        names = ["encoder." + n for n, _ in bert.named_parameters()]
        ipool = {names.index(POOL_W), names.index(POOL_B)}
        p0 = bert.pooler.weight.detach().clone()
        # a step on last_hidden_state alone: the pooler has no gradient, is not stepped and has no state
        bert(ids, attention_mask=mask).last_hidden_state.sum().backward()
        assert bert.pooler.weight.grad is None
        opt.step()
        assert not (ipool & set(opt.state_dict()["state"])) and torch.equal(bert.pooler.weight.detach(), p0)
        opt.zero_grad()
        ((cls(bert(ids, attention_mask=mask).pooler_output) - target) ** 2).mean().backward()
        opt.step()
        state = opt.state_dict()["state"]
        assert ipool <= set(state) and float(state[names.index(POOL_W)]["step"]) == 2.0
        assert not torch.equal(bert.pooler.weight.detach(), p0)
        bert2 = _bert(pcfg, sd, ids, finetune=True, train_pooler=True)
        opt2 = make(bert2)
        opt2.load_state_dict(opt.state_dict())
        for i in ipool:
            assert torch.equal(opt2.state_dict()["state"][i]["exp_avg_sq"], state[i]["exp_avg_sq"])


def _profiled(fn):
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    _lib.profile_read()
    fn()
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    return {k: v["launches"] for k, v in prof.items()}


def test_opt_in_off_is_the_plain_encode_backward():
    g, pcfg, sd, ids, mask = _fixture()
    bert = _bert(pcfg, sd, ids, finetune=True)
    assert bert.train_pooler is False
    eng = bert.engine
    out = bert(ids, attention_mask=mask)
    assert out.last_hidden_state.requires_grad and not out.pooler_output.requires_grad and out.pooler_output.grad_fn is None
    G = torch.as_tensor(np.random.RandomState(3).randn(3, 40, pcfg.hidden_size) * 1e-2, dtype=torch.float32).to(DEV)
    eng.grads.fill_(7.0)
    through_the_module = _profiled(lambda: out.last_hidden_state.backward(G))
    got = eng.grads.clone()
    assert bert.pooler.weight.grad is None and bert.pooler.bias.grad is None
    eng.encode(ids, mask.sum(1).to(torch.int32))
    eng.grads.fill_(7.0)
    through_the_engine = _profiled(lambda: eng.encode_bwd(G))
    assert torch.equal(_bits(got), _bits(eng.grads))
    assert through_the_module == through_the_engine and sum(through_the_engine.values()) > 10
    p0 = eng.layout[POOL_W][0]
    assert bool((got[p0:] == 7.0).all())                      # the pooler range is written by neither
    # the attribute on a wrapped encoder: off by default, on when set
    model = PhonemeOnlyModel(AlbertModel(pcfg, max_batch=3, max_seq=40), int(g["num_phonemes"]), pcfg.hidden_size)
    model.engine.load_state_dict(sd)
    enc = model.encoder
    enc.differentiable = True
    assert not enc(ids, attention_mask=mask).pooler_output.requires_grad
    enc.train_pooler = True
    o2 = enc(ids, attention_mask=mask)
    assert o2.pooler_output.requires_grad
    o2.pooler_output.sum().backward()
    assert enc.pooler.weight.grad is not None and model.phoneme_predictor.weight.grad is None
    # with the flag on, a backward that brings no gradient of pooler_output is the plain call too
    bert.train_pooler = True
    bert.zero_grad()                                          # (.grad holds views of engine.grads: a second backward would add in place)
    out = bert(ids, attention_mask=mask)
    eng.grads.fill_(7.0)
    flag_on_unused = _profiled(lambda: out.last_hidden_state.backward(G))
    assert torch.equal(_bits(got), _bits(eng.grads)) and flag_on_unused == through_the_engine
    assert bert.pooler.weight.grad is None
