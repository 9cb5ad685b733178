"""Host-side checks of the differentiable encoder (include/plbert.h: plb_encode / plb_encode_bwd) that need no GPU: the
library built for gfx950 exports the entry points and the new launcher, header and ctypes binding agree on their
signatures, and plbert_amd.train.AdamW exposes torch's ``param_groups`` over its live hyper-parameters."""
import ctypes as C

import c_header
from plbert_amd import _lib

ENTRY_POINTS = ("plb_encode", "plb_encode_bwd")


def test_library_exports_the_encode_entry_points():
    L = _lib.lib()   # (the in-tree build for gfx950; raises when it is missing)
    for s in ENTRY_POINTS:
        assert s in _lib.PUBLIC_SYMBOLS and hasattr(L, s), s
    for s in ("plb_launch_seed_dy", "plb_launch_unpack_rows"):
        assert hasattr(L, s), s


def test_header_and_binding_agree_on_the_signatures():
    L = _lib.lib()
    hdr, khdr = c_header.public(), c_header.kernels()
    for name in ENTRY_POINTS:
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert c_header.bound_mismatch(hdr, fn, _lib) is None
    # both take (engine, ids, lengths, B, S, packing, buffer, stream); the plan is a PlbPacking pointer
    for name, buf in (("plb_encode", "float* hidden"), ("plb_encode_bwd", "const float* d_hidden")):
        params = c_header.c_params(hdr, name)
        assert params[0] == "PlbEngine* e" and params[5] == "const PlbPacking* packing" and params[6] == buf, params
        assert params[-1] == "void* stream" and len(params) == 8
        assert getattr(L, name).argtypes[5] is C.POINTER(_lib.PlbPacking)
    params = c_header.c_params(khdr, "plb_launch_seed_dy")
    assert c_header.bound_mismatch(khdr, L.plb_launch_seed_dy, _lib) is None
    assert len(params) == 9 and params[0] == "const float* d_hidden" and params[7] == "bf16_t* dy"


class _StubEngine:
    """What train.AdamW touches: the layout, the trainable range, the flat gradient buffer and adamw_step."""

    def __init__(self, names):
        import torch
        self.layout = {n: (4 * i, 4, (4,)) for i, n in enumerate(names)}
        self.trainable = 4 * len(names)
        self.token_range = (self.trainable, self.trainable)
        self.grads = torch.zeros(self.trainable)
        self.exp_avg, self.exp_avg_sq = torch.zeros(self.trainable), torch.zeros(self.trainable)
        self.num_tokens, self.token_head_steps = 0, 0
        self._on_handoff_timeout = []
        self.calls = []

    def adamw_step(self, step, lr, betas, eps, weight_decay, grad_scale=1.0, norm_buf=None):
        self.calls.append(dict(step=step, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))


def test_adamw_param_groups_is_the_live_defaults():
    import torch
    from torch import nn

    from plbert_amd.train import AdamW

    class Model(nn.Module):   # a stand-alone encoder: parameter names lack the layout's "encoder." prefix
        def __init__(self):
            super().__init__()
            self.a = nn.Parameter(torch.zeros(4))
            self.b = nn.Parameter(torch.zeros(4))
            self.engine = _StubEngine(["encoder.a", "encoder.b"])

    m = Model()
    opt = AdamW(m.parameters(), lr=1e-3, model=m)
    assert opt._names == ["encoder.a", "encoder.b"]
    groups = opt.param_groups
    assert isinstance(groups, list) and len(groups) == 1 and groups[0] is opt.defaults
    assert groups[0]["lr"] == 1e-3 and groups[0]["weight_decay"] == 0.01
    for p in m.parameters():
        p.grad = torch.ones(4)
    opt.step()
    for g in opt.param_groups:   # the reference README's fine-tuning set-up
        g["lr"] = 1e-5
        g["betas"] = (0.9, 0.99)
        g["weight_decay"] = 0.1
    opt.step()
    eng = m.engine
    assert [c["lr"] for c in eng.calls] == [1e-3, 1e-5] and [c["step"] for c in eng.calls] == [1, 2]
    assert eng.calls[1]["betas"] == (0.9, 0.99) and eng.calls[1]["weight_decay"] == 0.1
    assert opt.state_dict()["param_groups"][0]["lr"] == 1e-5


def test_albert_model_takes_the_finetune_switch():
    import inspect

    from plbert_amd.model import AlbertModel
    sig = inspect.signature(AlbertModel.__init__)
    assert sig.parameters["finetune"].default is False
