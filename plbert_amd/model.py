"""Host-side mirror of the reference model interface, backed by the HIP engine.

Same names, constructor arguments and call conventions as the reference so its callers keep
working:

* ``AlbertModel(AlbertConfig(vocab_size=len(symbols), **config['model_params']))``  (train.py:263-265)
* ``PhonemeOnlyModel(model, num_phonemes, hidden_size)``                            (model.py:19-30)
* ``MultiTaskModel(model, num_phonemes, num_tokens, hidden_size)``                  (model.py:5-18)
* ``model(phonemes, attention_mask=(~text_mask).int())``                             (train.py:386)
* ``encoder(ids, attention_mask=...).last_hidden_state``                             (README.md:91)
* ``.parameters()`` / ``.state_dict()`` / ``.load_state_dict(strict=False)`` with the reference key
  names, ``.train()`` / ``.eval()``                                                 (train.py:100,272,290,417)

The modules are real ``torch.nn.Module`` trees whose Parameters are VIEWS into the engine's flat fp32
buffer, so ``load_state_dict``/``state_dict``/``torch.save`` behave as usual while the kernels see
one contiguous allocation.  Forward runs entirely in libplbert_hip.so (no autograd graph: outputs
are plain tensors; training goes through ``loss_and_grads`` / ``plbert_amd.train``).

Fine-tuning inside a downstream model (the reference README's "Finetuning" section) is the one place
where a forward joins torch's autograd graph: an encoder whose ``differentiable`` attribute is set
(``AlbertModel(config, finetune=True)``, or ``model.encoder.differentiable = True`` on a wrapped one)
returns a ``last_hidden_state`` that requires grad while the module is in training mode and grad is
enabled; ``backward()`` runs plb_encode_bwd and hands every encoder Parameter its slice of the
engine's gradient buffer.  ``pooler_output`` is returned DETACHED (the pooler gets no gradient) unless the encoder's
``train_pooler`` attribute is set (``AlbertModel(config, finetune=True, train_pooler=True)``): then it joins the graph too — a
loss on it reaches the pooler's two Parameters and, through position 0 of the last hidden state, the encoder
(plb_encode_bwd_pooled).  ``last_hidden_state`` is zero at pad positions.

``attention_mask`` of ``AlbertModel.forward`` follows transformers' 2-D rule and need not be a prefix (left padding, keys
knocked out, a sub-span of a buffer): key j of a sample takes part in the softmax of all its queries iff its entry is nonzero.
A prefix mask runs the lengths-only kernels as before; any other mask goes through plb_forward_masked / plb_encode_masked /
plb_encode_bwd_masked with the sample's EXTENT (1 + its last valid position) as its length. Positions at or past the extent
are pad positions (zeros); a masked position below it is a hole, removed as a key only — it has a hidden state and carries
gradient, as in transformers. The head wrappers, ``fill_mask``, ``predict_tokens`` and the trainer take prefix masks only.

``output_hidden_states=True`` / ``output_attentions=True`` (transformers' arguments of ``AlbertModel.forward``) add
``.hidden_states`` (the model after every application of the shared layer) and ``.attentions``; on the differentiable
path every hidden state joins the graph (plb_encode_layers / plb_encode_bwd_layers), elsewhere plb_forward_layers runs.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import torch
from torch import nn

from .engine import HipEngine
from .init import reference_init_state_dict

_DEFAULT_MAX_BATCH = 32


@dataclass
class BaseModelOutputWithPooling:
    last_hidden_state: torch.Tensor
    pooler_output: torch.Tensor | None = None
    hidden_states: tuple | None = None   # output_hidden_states=True: L + 1 tensors, [0] = the map-in output, [-1] IS last_hidden_state
    attentions: tuple | None = None      # output_attentions=True: L tensors [B,NH,S,S]

    def to_tuple(self):
        """The fields that are not None, in order (transformers' ModelOutput.to_tuple)."""
        return tuple(v for v in (self.last_hidden_state, self.pooler_output, self.hidden_states, self.attentions)
                     if v is not None)

    def __getitem__(self, i):
        return self.to_tuple()[i]


class _Leaf(nn.Module):
    """Holds ``weight`` (and ``bias``) Parameters under the reference's attribute names."""

    def __init__(self, weight, bias=None):
        super().__init__()
        self.weight = nn.Parameter(weight, requires_grad=True)
        if bias is not None:
            self.bias = nn.Parameter(bias, requires_grad=True)


def _packing_from_lengths(module, lengths, ids):
    """Token-packed forward (include/plbert.h: plb_forward_packed) when the module's ``packed`` attribute — default:
    PLBERT_PACKED=1 — is set and the mask pads anything: the plan is made on the host from the mask's lengths (one small
    read-back here; a caller that has the lengths on the host passes ``packing`` to HipEngine.forward itself). Outputs
    at pad positions are then zeros."""
    from .train import make_packing
    packed = getattr(module, "packed", None)
    if lengths is None or not (packed if packed is not None else os.environ.get("PLBERT_PACKED", "0") == "1"):
        return None
    return make_packing(lengths.cpu().numpy(), ids.shape[1], module.engine.device, True)


def _lengths_from_mask(attention_mask, strict=True):
    """int [B,S] with 1 = valid -> int32 lengths. The kernels mask keys by length, so the mask must be
    a prefix mask (what train.py:384-386 builds from input_lengths)."""
    if attention_mask is None:
        return None
    am = attention_mask != 0
    lengths = am.sum(dim=1).to(torch.int32)
    if strict:
        S = am.shape[1]
        prefix = torch.arange(S, device=am.device)[None, :] < lengths[:, None]
        if not bool((prefix == am).all()):
            raise ValueError("attention_mask must mark a prefix of each row (1...1 0...0): the HIP attention "
                             "kernels take per-sample lengths")
        if bool((lengths < 1).any()):
            raise ValueError("attention_mask has a row with no valid token")
    return lengths


def _extent_from_mask(attention_mask):
    """int [B,S], nonzero = attend -> (extent int32 [B] = 1 + the last valid position of each row, whether every row is a
    prefix 1...1 0...0). torch ops on the mask's device, one read-back for the two flags. A row without a valid token
    raises ValueError."""
    am = attention_mask != 0
    if am.dim() != 2:
        raise ValueError(f"attention_mask must be [B,S], got {tuple(am.shape)}")
    S = am.shape[1]
    extent = (am * torch.arange(1, S + 1, device=am.device)[None, :]).amax(dim=1).to(torch.int32)
    empty, prefix = torch.stack([(extent < 1).any(), (am.sum(dim=1) == extent).all()]).tolist()
    if empty:
        raise ValueError("attention_mask has a row with no valid token")
    return extent, bool(prefix)


def _lengths_and_key_mask(attention_mask):
    """AlbertModel.forward's reading of its mask: (lengths | None, key mask | None). A prefix mask gives the lengths alone
    (the path without a key mask); any other mask gives its extents and itself."""
    if attention_mask is None:
        return None, None
    extent, prefix = _extent_from_mask(attention_mask)
    return extent, (None if prefix else attention_mask)


_POOLER_NAMES = ("encoder.pooler.weight", "encoder.pooler.bias")


class _Encode(torch.autograd.Function):
    """The differentiable forward as ONE autograd node, whatever the call carries: HipEngine.encode / encode_bwd choose the
    entry points (plb_encode / plb_encode_bwd for the plain call, the _layers / _inputs / _masked rungs for the rest). The
    engine keeps ONE forward's activations: the backward of a forward that a later engine call has overwritten raises.
    Outputs: the L + 1 hidden states (``want_hs``; else the last hidden state alone), then the L attention maps (``want_at``),
    which are marked non-differentiable. The backward hands the gradient of the last slot to the engine as d_hidden and those
    of the slots below as d_below; a slot nothing downstream used arrives as None and goes in as a NULL pointer. Every encoder
    Parameter receives the view of its slice of ``engine.grads`` (the scheme of train._FusedLoss), the pooler and the heads
    receive None. ``train_pooler``: ``pooler_output`` (plb_pooler on the last hidden state) is one more output, the last one;
    when its gradient arrives it goes to the engine as d_pooled and the two pooler Parameters receive their views too; when it
    does not (None), the call and the Parameters' None are those of a forward without the flag. ``inputs_embeds`` (or None) is an input of the node: when it requires grad it receives the gradient of the
    pre-LayerNorm embedding sum, and the word table — which took no part — receives None, as in torch. ``key_mask`` (or
    None): a mask that is no prefix (the engine's live record hands it to the backward)."""

    @staticmethod
    def forward(ctx, engine, names, ids, lengths, packing, want_hs, want_at, token_type_ids, position_ids, inputs_embeds,
                key_mask, train_pooler, *params):
        layers = dict(hidden_states=want_hs, attentions=want_at) if want_hs or want_at else None
        out = engine.encode(ids, lengths, packing, layers=layers, token_type_ids=token_type_ids, position_ids=position_ids,
                            inputs_embeds=inputs_embeds, key_mask=key_mask)
        hid, hs, at = (out, None, None) if layers is None else out
        ctx.engine, ctx.names, ctx.serial, ctx.want_hs = engine, names, engine._encode_serial, want_hs
        ctx.embeds = inputs_embeds is not None
        ctx.pooled = bool(train_pooler)
        ctx.set_materialize_grads(False)
        if want_at:
            ctx.mark_non_differentiable(*at)
        return (*(hs if want_hs else [hid]), *(at if want_at else []), *([engine.pooler(hid)] if train_pooler else []))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        eng = ctx.engine
        nl = eng.cfg.num_hidden_layers
        g = [None if x is None else x.contiguous().float() for x in grads[:nl + 1 if ctx.want_hs else 1]]
        gp = grads[-1].contiguous().float() if ctx.pooled and grads[-1] is not None else None
        gone = "a later engine call overwrote the activations of this forward (the engine keeps one differentiable " \
               "forward at a time: call backward() before the next forward, loss call or optimizer step)"
        if eng._live_encode is None or eng._encode_serial != ctx.serial:
            raise RuntimeError(gone)
        try:
            die = eng.encode_bwd(g[-1], d_below=g[:-1] if ctx.want_hs else None,
                                 want_d_inputs_embeds=ctx.embeds and ctx.needs_input_grad[9], d_pooled=gp)
        except RuntimeError as ex:
            if "no live plb_encode stash" in str(ex):
                raise RuntimeError(f"{gone}: {ex}") from ex
            raise
        end = eng.layout["phoneme_predictor.weight"][0]   # the encoder range of the flat buffers
        without = ("encoder.embeddings.word_embeddings.weight",) if ctx.embeds else ()
        pg = []
        for n in ctx.names:
            off, size, shp = eng.layout[n]
            has = off + size <= end and n not in without or gp is not None and n in _POOLER_NAMES
            pg.append(eng.grads[off:off + size].view(shp) if has else None)
        return (None,) * 9 + (die, None, None) + tuple(pg)


class AlbertModel(nn.Module):
    """Drop-in for ``transformers.AlbertModel`` on this path (modeling_albert.py:338-408)."""

    def __init__(self, config, add_pooling_layer=True, max_batch=_DEFAULT_MAX_BATCH, max_seq=None, device=None, seed=0,
                 finetune=False, train_pooler=False):
        """``train_pooler=True`` (with ``finetune``; the attribute of the same name may be set later, also on a wrapped
        encoder): ``pooler_output`` of a differentiable forward carries gradient — into ``pooler.weight`` / ``pooler.bias``
        and, through position 0 of the last hidden state, into the encoder. Off (the default): it is detached.
        ``finetune=True``: the encoder sits on a TRAINING engine of its own and is ``differentiable`` — the model a TTS
        training loop fine-tunes (reference README "Finetuning": ``bert(texts, attention_mask=...).last_hidden_state``
        feeding the caller's layers, ``optimizer.step('bert')``)."""
        super().__init__()
        config.check_supported()
        self.config = config
        self._max_batch = max_batch
        self._max_seq = max_seq or config.max_position_embeddings
        self._device = device
        self._seed = seed
        self._engine = None
        # An encoder on its own is an inference model (README.md:91: bert(texts, attention_mask=...)): its engine holds
        # the parameters and, from the first forward on, one layer of activations (< 1 GB at 32 x 512) — no gradient,
        # moment or per-layer stash. Wrapped by PhonemeOnlyModel / MultiTaskModel its parameters move into the
        # wrapper's training engine before this one has allocated anything but them.
        # finetune: all layers' activations, gradients and AdamW moments (the stand-in head sizes stay: the head is unused)
        self.differentiable = bool(finetune)
        self.train_pooler = bool(train_pooler)
        self._build(HipEngine(config, 4, 0, max_batch=self._max_batch, max_seq=self._max_seq, device=device,
                              train=bool(finetune)),
                    reference_init_state_dict(config, 4, 0, seed=seed), prefix="encoder.")

    # -- module tree with the reference's parameter names ----------------------------------------------
    def _build(self, engine, init_sd, prefix):
        """(Re)create the Parameter views over ``engine``'s flat buffer."""
        v = lambda name: engine.view(prefix + name)
        self._engine = engine
        if init_sd is not None:
            engine.load_state_dict({k: t for k, t in init_sd.items() if k in engine.layout}, strict=False)
        emb = nn.Module()
        emb.word_embeddings = _Leaf(v("embeddings.word_embeddings.weight"))
        emb.position_embeddings = _Leaf(v("embeddings.position_embeddings.weight"))
        emb.token_type_embeddings = _Leaf(v("embeddings.token_type_embeddings.weight"))
        emb.LayerNorm = _Leaf(v("embeddings.LayerNorm.weight"), v("embeddings.LayerNorm.bias"))
        self.embeddings = emb
        lp = "encoder.albert_layer_groups.0.albert_layers.0."
        layer = nn.Module()
        layer.full_layer_layer_norm = _Leaf(v(lp + "full_layer_layer_norm.weight"), v(lp + "full_layer_layer_norm.bias"))
        att = nn.Module()
        for nm in ("query", "key", "value", "dense", "LayerNorm"):
            setattr(att, nm, _Leaf(v(lp + f"attention.{nm}.weight"), v(lp + f"attention.{nm}.bias")))
        layer.attention = att
        layer.ffn = _Leaf(v(lp + "ffn.weight"), v(lp + "ffn.bias"))
        layer.ffn_output = _Leaf(v(lp + "ffn_output.weight"), v(lp + "ffn_output.bias"))
        group = nn.Module()
        group.albert_layers = nn.ModuleList([layer])
        enc = nn.Module()
        enc.embedding_hidden_mapping_in = _Leaf(v("encoder.embedding_hidden_mapping_in.weight"),
                                                v("encoder.embedding_hidden_mapping_in.bias"))
        enc.albert_layer_groups = nn.ModuleList([group])
        self.encoder = enc
        self.pooler = _Leaf(v("pooler.weight"), v("pooler.bias"))

    def _adopt(self, engine, owner):
        """Called by a head wrapper: move this encoder's values into the wrapper's engine."""
        old = {"encoder." + k: p.detach().clone() for k, p in self.state_dict().items()}
        self._build(engine, None, prefix="encoder.")
        engine.load_state_dict(old, strict=False)

    @property
    def engine(self):
        return self._engine

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None,
                output_hidden_states=False, output_attentions=False, inputs_embeds=None, **unused):
        """``output_hidden_states`` / ``output_attentions`` (transformers' arguments): ``.hidden_states`` = L + 1 tensors
        [B,S,H] (the output of embedding_hidden_mapping_in, then of every application of the shared layer; the last one IS
        ``last_hidden_state``), ``.attentions`` = L tensors [B,NH,S,S]. Pad positions of the hidden states, pad query rows
        and pad key columns of the attention maps are ZEROS (transformers leaves values in pad rows). On the differentiable
        path every hidden state carries gradient; the attention maps never do.
        ``token_type_ids`` [B,S], ``position_ids`` [B,S] or [1,S], ``inputs_embeds`` [B,S,embedding_size] instead of
        ``input_ids`` (transformers' arguments and rules; AlbertEmbeddings.forward with dropout 0): on the differentiable
        path an ``inputs_embeds`` that requires grad receives its gradient, and the word table's ``.grad`` stays None.
        ``attention_mask`` [B,S], nonzero = attend (transformers' 2-D key-padding rule): a prefix mask runs as it always
        did; any other mask — left padding, holes — runs the masked attention kernels (module docstring). Positions at or
        past a row's last valid token are pad positions (zeros); a hole below it keeps its hidden state and its gradient and
        has an all-zero column in every attention map. A row without a valid token raises ValueError."""
        if (input_ids is None) == (inputs_embeds is None):
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
        lengths, key_mask = _lengths_and_key_mask(attention_mask)
        pooled = None
        want_hs, want_at = bool(output_hidden_states), bool(output_attentions)
        nl, eng = self.config.num_hidden_layers, self._engine
        given = {k: v for k, v in dict(token_type_ids=token_type_ids, position_ids=position_ids, inputs_embeds=inputs_embeds,
                                       key_mask=key_mask).items() if v is not None}
        packing = _packing_from_lengths(self, lengths, input_ids if input_ids is not None else inputs_embeds)
        if getattr(self, "differentiable", False) and self.training and torch.is_grad_enabled():
            # fine-tuning: the forward joins the autograd graph (_Encode); pad positions of last_hidden_state are zeros and
            # pooler_output is DETACHED (the pooler receives no gradient) unless train_pooler makes it an output of the node
            pool_grad = bool(getattr(self, "train_pooler", False))
            names, params = [], []
            for n, p in self.named_parameters():
                names.append("encoder." + n)
                params.append(p)
            outs = _Encode.apply(eng, names, input_ids, lengths, packing, want_hs, want_at, token_type_ids, position_ids,
                                 inputs_embeds, key_mask, pool_grad, *params)
            pooled, outs = (outs[-1], outs[:-1]) if pool_grad else (None, outs)
            hs = tuple(outs[:nl + 1]) if want_hs else None
            at = tuple(outs[-nl:]) if want_at else None
            hid = hs[-1] if want_hs else outs[0]
        elif want_hs or want_at or given:
            # (the engine checks shapes and index ranges of the embedding inputs; ``lengths`` of a mask that is no prefix are
            # its extents)
            hs, at, hid = eng.forward_layers(input_ids, lengths, packing, hidden_states=want_hs, attentions=want_at,
                                             want_hidden=True, **given)
            if want_hs:
                hid = hs[-1]   # (the same tensor object, as in transformers; unlike `hidden`, zeros at pad positions)
            hs, at = tuple(hs) if want_hs else None, tuple(at) if want_at else None
        else:
            (hid, _, _), hs, at = eng.forward(input_ids, lengths, want_hidden=True, want_phoneme=False, packing=packing), None, None
        # pooler (modeling_albert.py:403): computed for API completeness (plb_pooler), never used by the loss; the pooler of
        # position 0, hole or not, as in transformers
        if pooled is None:
            pooled = eng.pooler(hid.detach())
        return BaseModelOutputWithPooling(last_hidden_state=hid, pooler_output=pooled, hidden_states=hs, attentions=at)


class _HeadModel(nn.Module):
    def __init__(self, model, num_phonemes, num_tokens, hidden_size):
        super().__init__()
        if not isinstance(model, AlbertModel):
            raise TypeError("model must be a plbert_amd.AlbertModel")
        if hidden_size != model.config.hidden_size:
            raise ValueError("hidden_size does not match the encoder")
        cfg = model.config
        engine = HipEngine(cfg, num_phonemes, num_tokens, max_batch=model._max_batch, max_seq=model._max_seq,
                           device=model._device)
        init = reference_init_state_dict(cfg, num_phonemes, num_tokens, seed=model._seed)
        engine.load_state_dict({k: v for k, v in init.items() if not k.startswith("encoder.")}, strict=False)
        model._adopt(engine, self)
        self.encoder = model
        self.phoneme_predictor = _Leaf(engine.view("phoneme_predictor.weight"), engine.view("phoneme_predictor.bias"))
        if num_tokens:
            self.token_predictor = _Leaf(engine.view("token_predictor.weight"), engine.view("token_predictor.bias"))
        self._engine = engine

    @property
    def engine(self):
        return self._engine

    def fill_mask(self, phonemes, positions, attention_mask=None, topk=5):
        """The model's predictions at chosen positions: ``phonemes`` int64 [B,S] (the input as the model is to see it,
        mask tokens included), ``positions`` one list of positions per sample (inside the sample's valid length, no
        position twice). Returns ``(ids int64 [n, topk], probs fp32 [n, topk])`` on the device, n = all listed positions in
        the order given, classes by descending probability (among equal logits the lowest id first). One loss-only call
        whose labels are the ids themselves (plb_loss_fwd: works in eval mode and on an inference-only engine) followed by
        the report on the rows it left (plb_masked_report); no [B,S,num_phonemes] logits are materialised."""
        import numpy as np
        from .data import masked_indices_to_csr
        eng = self._engine
        ids = eng._dev_i64(phonemes)
        B, S = ids.shape
        if len(positions) != B:
            raise ValueError(f"fill_mask: {len(positions)} position lists for {B} samples")
        lengths = _lengths_from_mask(attention_mask)
        lens = [S] * B if lengths is None else lengths.cpu().tolist()
        for b, (idx, ln) in enumerate(zip(positions, lens)):
            a = np.asarray(idx, dtype=np.int64).reshape(-1)
            if a.size and (a.min() < 0 or a.max() >= ln):
                raise ValueError(f"fill_mask: sample {b}: position outside [0, {ln})")
            if len(np.unique(a)) != a.size:
                raise ValueError(f"fill_mask: sample {b}: duplicate position")
        off, flat = masked_indices_to_csr([np.asarray(idx, dtype=np.int64).reshape(-1) for idx in positions])
        n = int(off[-1])
        if n == 0:
            return (torch.empty((0, topk), dtype=torch.int64, device=eng.device),
                    torch.empty((0, topk), dtype=torch.float32, device=eng.device))
        offs = torch.from_numpy(off).to(eng.device)
        eng.loss_fwd(ids, ids, lengths, offs, torch.from_numpy(flat).to(eng.device), n)
        rep = eng.masked_report(offs, topk=topk, want=("topk_ids", "topk_logprob"))
        return rep["topk_ids"].to(torch.int64), rep["topk_logprob"].exp()


class PhonemeOnlyModel(_HeadModel):
    """model.py:19-30 — ``forward(phonemes, attention_mask=None) -> phoneme_pred`` (fp32 [B,S,num_phonemes])."""

    def __init__(self, model, num_phonemes, hidden_size):
        super().__init__(model, num_phonemes, 0, hidden_size)

    def forward(self, phonemes, attention_mask=None):
        lengths = _lengths_from_mask(attention_mask)
        _, ph, _ = self._engine.forward(phonemes, lengths, packing=_packing_from_lengths(self, lengths, phonemes))
        return ph


class MultiTaskModel(_HeadModel):
    """model.py:5-18 — ``forward(phonemes, attention_mask=None) -> (phoneme_pred, token_pred)``."""

    def __init__(self, model, num_phonemes, num_tokens, hidden_size):
        super().__init__(model, num_phonemes, num_tokens, hidden_size)

    def forward(self, phonemes, attention_mask=None):
        _, ph, tk = self._engine.forward(phonemes, _lengths_from_mask(attention_mask), want_token=True)
        return ph, tk

    def predict_tokens(self, phonemes, attention_mask=None, positions=None, topk=5):
        """The token (grapheme) head's predictions: ``phonemes`` int64 [B,S], ``positions`` one list of positions per sample
        (inside the sample's valid length) or None = every valid position. Returns ``(ids int64 [n, topk], probs fp32
        [n, topk])`` on the device, n = the positions in (sample, position) order, classes by descending probability (among
        equal logits the lowest id first; -1 / 0 behind num_tokens). One forward that outputs nothing (it honours ``packed``
        like ``PhonemeOnlyModel.forward``; works in eval mode and on an inference-only engine) followed by the fused
        top-k over the vocabulary (plb_token_report): no [B,S,num_tokens] logits are materialised, unlike ``forward``."""
        import numpy as np
        from .data import masked_indices_to_csr
        eng = self._engine
        ids = eng._dev_i64(phonemes)
        B, S = ids.shape
        lengths = _lengths_from_mask(attention_mask)
        lens = [S] * B if lengths is None else [min(max(int(v), 1), S) for v in lengths.cpu().tolist()]
        if positions is None:
            positions = [np.arange(ln, dtype=np.int64) for ln in lens]
        if len(positions) != B:
            raise ValueError(f"predict_tokens: {len(positions)} position lists for {B} samples")
        lists = [np.asarray(idx, dtype=np.int64).reshape(-1) for idx in positions]
        for b, (a, ln) in enumerate(zip(lists, lens)):
            if a.size and (a.min() < 0 or a.max() >= ln):
                raise ValueError(f"predict_tokens: sample {b}: position outside [0, {ln})")
        off, flat = masked_indices_to_csr(lists)
        if int(off[-1]) == 0:
            return (torch.empty((0, topk), dtype=torch.int64, device=eng.device),
                    torch.empty((0, topk), dtype=torch.float32, device=eng.device))
        eng.forward(ids, lengths, want_hidden=False, want_phoneme=False, want_token=False,
                    packing=_packing_from_lengths(self, lengths, ids))
        rep = eng.token_report((torch.from_numpy(off), torch.from_numpy(flat)), topk=topk, want=("topk_ids", "topk_logprob"))
        return rep["topk_ids"].to(torch.int64), rep["topk_logprob"].exp()
