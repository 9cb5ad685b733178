"""Token-packed calls in fp8 mode, host side (no GPU): the header declares the switch, the library built for gfx950 exports
it (the linker script keeps every extern "C" entry point global), the ctypes binding agrees with the declaration,
PLBERT_PACKED_FP8 is read the way the other environment switches are, and the engine, the trainer and run.py carry the
setting."""
import ctypes as C
import inspect
import os
import re

import pytest

from plbert_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_declares_the_switch_and_its_semantics():
    hdr = _read("include", "plbert.h")
    m = re.search(r"\bint\s+plb_set_packed_fp8\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["PlbEngine* e", "int32_t on"]
    block = hdr[:m.start()].rsplit("/*", 1)[1]
    for words in ("Site maxima", "Tile forms", "plb_set_packed_dual", "plb_encode keeps refusing"):
        assert words in block, words
    assert "fp8 mode always runs padded" not in hdr


def test_library_exports_the_switch_and_the_binding_agrees():
    L = _lib.lib()   # (the in-tree build for gfx950; raises when it is missing)
    assert "plb_set_packed_fp8" in _lib.PUBLIC_SYMBOLS and hasattr(L, "plb_set_packed_fp8")
    assert L.plb_set_packed_fp8.restype is C.c_int
    assert list(L.plb_set_packed_fp8.argtypes) == [C.c_void_p, C.c_int32]
    # the version script hides hipcc's per-unit markers only: no global list that could leave the new symbol out
    assert "global:" not in _read("plbert_amd", "csrc", "exports.map")
    # a null engine is refused on the host, nothing else is touched
    assert L.plb_set_packed_fp8(None, 1) != 0
    assert b"plb_set_packed_fp8" in L.plb_last_error()


def test_embedding_launch_struct_matches_the_kernel_header():
    """PlbEmbed gained the fill_slots flag behind B (in what was tail padding: the size is unchanged)."""
    khdr = _read("plbert_amd", "csrc", "plbert_kernels.h")
    assert re.search(r"const int32_t\* row_start; const int32_t\* lengths; int B; int fill_slots;\s*\} PlbEmbed;", khdr)
    names = [f[0] for f in _lib.PlbEmbed._fields_]
    assert names[-2:] == ["B", "fill_slots"]
    assert C.sizeof(_lib.PlbEmbed) % 8 == 0 and _lib.PlbEmbed.fill_slots.offset == _lib.PlbEmbed.B.offset + 4


@pytest.mark.parametrize("value,on", [(None, False), ("1", True), ("0", False), ("", False), (" 1 ", True), ("true", False),
                                      ("2", False)])
def test_environment_switch(monkeypatch, value, on):
    from plbert_amd.engine import packed_fp8_default
    if value is None:
        monkeypatch.delenv("PLBERT_PACKED_FP8", raising=False)
    else:
        monkeypatch.setenv("PLBERT_PACKED_FP8", value)
    assert packed_fp8_default() is on


def test_engine_trainer_and_run_carry_the_switch():
    from plbert_amd.engine import HipEngine
    from plbert_amd.train import PLBertTrainer
    assert inspect.signature(HipEngine.set_packed_fp8).parameters["on"].default is True
    assert inspect.signature(PLBertTrainer.__init__).parameters["packed_fp8"].default is None
    src = inspect.getsource(HipEngine.__init__)
    assert "packed_fp8_default()" in src and "self.packed_fp8 = False" in src


@pytest.mark.parametrize("setting", [None, True, False])
def test_run_hands_training_params_packed_fp8_to_the_trainer(monkeypatch, tmp_path, setting):
    """run.initialize_model with a stand-in trainer: training_params.packed_fp8 arrives as the trainer's packed_fp8 (a
    missing key as None: the engine's own reading of PLBERT_PACKED_FP8 stands), beside packed_dual."""
    from plbert_amd import run, train
    got = {}

    class FakeTrainer:
        def __init__(self, cfg, **kw):
            got.update(kw)

    monkeypatch.setattr(train, "PLBertTrainer", FakeTrainer)
    monkeypatch.setattr(run, "albert_config_from_yaml", lambda config, n: None)
    tp = {"batch_size": 4, "learning_rate": 1e-4, "packed_dual": True}
    if setting is not None:
        tp["packed_fp8"] = setting
    config = {"training_params": tp, "dataset_params": {"max_seq_length": 128}, "model_params": {}}
    trainer, step = run.initialize_model(config, str(tmp_path), resuming=False)
    assert isinstance(trainer, FakeTrainer) and step == 0
    assert got["packed_fp8"] is setting and got["packed_dual"] is True


def test_trainer_passes_the_setting_to_its_engine(monkeypatch):
    """PLBertTrainer without a GPU: a stand-in engine records what the constructor hands on (None: the engine's own
    reading of PLBERT_PACKED_FP8 stands)."""
    from plbert_amd import train

    class Stop(Exception):
        pass

    class FakeEngine:
        def __init__(self, *a, **kw):
            self.packed_dual, self.packed_fp8, self.calls, self.device = False, "from the environment", [], "cpu"

        def set_packed_dual(self, on):
            self.packed_dual = bool(on)

        def set_packed_fp8(self, on):
            self.calls.append(on)
            self.packed_fp8 = bool(on)

    seen = {}

    def stop(*a, **kw):
        raise Stop

    monkeypatch.setattr(train, "HipEngine", FakeEngine)
    monkeypatch.setattr(train, "GradReducer", stop)
    for arg, want in ((None, "from the environment"), (True, True), (False, False)):
        tr = train.PLBertTrainer.__new__(train.PLBertTrainer)
        with pytest.raises(Stop):
            tr.__init__(None, 188, packed=True, packed_fp8=arg)
        seen[arg] = (tr.packed_fp8, tr.engine.calls)
        assert tr.packed_fp8 == want and tr.engine.calls == ([] if arg is None else [arg])
