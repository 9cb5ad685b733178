"""Token-packed dual-head calls, host side (no GPU): the library built for gfx950 exports the switch, the new entry point
and the two launchers of the packed token head; header and ctypes binding agree on their signatures; PLBERT_PACKED_DUAL is
read the way the other environment switches are; the trainer and the engine carry the switch."""
import ctypes as C
import inspect

import pytest

import c_header
from plbert_amd import _lib

ENTRY_POINTS = ("plb_set_packed_dual", "plb_loss_fwd_bwd_dual_packed")
LAUNCHERS = ("plb_launch_pack_token_targets", "plb_launch_token_ce_combine_packed")


def test_library_exports_the_packed_dual_entry_points():
    L = _lib.lib()   # (the in-tree build for gfx950; raises when it is missing)
    for s in ENTRY_POINTS:
        assert s in _lib.PUBLIC_SYMBOLS and hasattr(L, s), s
    for s in LAUNCHERS:
        assert hasattr(L, s), s


def test_header_and_binding_agree_on_the_signatures():
    L = _lib.lib()
    hdr, khdr = c_header.public(), c_header.kernels()
    _c_params = c_header.c_params
    for header, names in ((hdr, ENTRY_POINTS), (khdr, LAUNCHERS)):
        for name in names:
            fn = getattr(L, name)
            assert fn.restype is C.c_int
            assert c_header.bound_mismatch(header, fn, _lib) is None
    assert _c_params(hdr, "plb_set_packed_dual") == ["PlbEngine* e", "int32_t on"]
    # plb_loss_fwd_bwd_dual with a plan in front of the outputs
    dual, packed = _c_params(hdr, "plb_loss_fwd_bwd_dual"), _c_params(hdr, "plb_loss_fwd_bwd_dual_packed")
    assert packed[:10] == dual[:10] and packed[10] == "const PlbPacking* packing" and packed[11:] == dual[10:]
    assert L.plb_loss_fwd_bwd_dual_packed.argtypes[10] is C.POINTER(_lib.PlbPacking)
    params = _c_params(khdr, "plb_launch_pack_token_targets")
    assert params[0] == "const int64_t* token_ids" and params[6] == "int64_t* out" and len(params) == 8
    params = _c_params(khdr, "plb_launch_token_ce_combine_packed")
    assert len(params) == 13 and params[5] == "const int32_t* row_start"


@pytest.mark.parametrize("value,on", [(None, False), ("1", True), ("0", False), ("", False), (" 1 ", True), ("true", False),
                                      ("2", False)])
def test_environment_switch(monkeypatch, value, on):
    from plbert_amd.engine import packed_dual_default
    if value is None:
        monkeypatch.delenv("PLBERT_PACKED_DUAL", raising=False)
    else:
        monkeypatch.setenv("PLBERT_PACKED_DUAL", value)
    assert packed_dual_default() is on


def test_engine_and_trainer_carry_the_switch():
    from plbert_amd.engine import HipEngine
    from plbert_amd.train import PLBertTrainer
    assert inspect.signature(HipEngine.set_packed_dual).parameters["on"].default is True
    assert inspect.signature(PLBertTrainer.__init__).parameters["packed_dual"].default is None
