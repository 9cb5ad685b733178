"""Host: the entry-point tables of plbert_amd/engine.py (encoder_entry, loss_entry, ENTRY_ARGS). No GPU, no library.

HipEngine picks the C symbol of an encoder or loss call with two pure functions and passes the arguments of that symbol in
the order ENTRY_ARGS lists, every one of them through c_void_p. Two checks stand where the compiler cannot:
  * the selection: for every combination of what a caller can give, the symbol is the one the if-chains this table replaced
    reached (literals below, written from those chains);
  * the order: for every symbol of the table, the names equal the parameter names of its prototype in include/plbert.h.
"""
import itertools

import pytest

import c_header
from plbert_amd import _lib
from plbert_amd.engine import ENTRY_ARGS, encoder_entry, loss_entry

# (per-application outputs given, embedding inputs given, key mask given) -> symbol
FORWARD = {   # (the plain rung is HipEngine.forward's; forward_layers always passes layers=True)
    (False, False, False): "plb_forward", (True, False, False): "plb_forward_layers",
    (False, True, False): "plb_forward_inputs", (True, True, False): "plb_forward_inputs",
    (False, False, True): "plb_forward_masked", (True, False, True): "plb_forward_masked",
    (False, True, True): "plb_forward_masked", (True, True, True): "plb_forward_masked",
}
ENCODE = {
    (False, False, False): "plb_encode", (True, False, False): "plb_encode_layers",
    (False, True, False): "plb_encode_inputs", (True, True, False): "plb_encode_inputs",
    (False, False, True): "plb_encode_masked", (True, False, True): "plb_encode_masked",
    (False, True, True): "plb_encode_masked", (True, True, True): "plb_encode_masked",
}
# (embedding inputs of the live encode, its key mask, d_below given, want_d_inputs_embeds) -> symbol
ENCODE_BWD = {
    (False, False, False, False): "plb_encode_bwd", (False, False, True, False): "plb_encode_bwd_layers",
    (False, False, False, True): "plb_encode_bwd_inputs", (False, False, True, True): "plb_encode_bwd_inputs",
    (True, False, False, False): "plb_encode_bwd_inputs", (True, False, True, False): "plb_encode_bwd_inputs",
    (True, False, False, True): "plb_encode_bwd_inputs", (True, False, True, True): "plb_encode_bwd_inputs",
    (False, True, False, False): "plb_encode_bwd_masked", (False, True, True, False): "plb_encode_bwd_masked",
    (False, True, False, True): "plb_encode_bwd_masked", (False, True, True, True): "plb_encode_bwd_masked",
    (True, True, False, False): "plb_encode_bwd_masked", (True, True, True, False): "plb_encode_bwd_masked",
    (True, True, False, True): "plb_encode_bwd_masked", (True, True, True, True): "plb_encode_bwd_masked",
}
# (backward, dual-head, plan given) -> symbol
LOSS = {
    (False, False, False): "plb_loss_fwd", (False, True, False): "plb_loss_fwd",
    (False, False, True): "plb_loss_fwd_packed", (False, True, True): "plb_loss_fwd_packed",
    (True, False, False): "plb_loss_fwd_bwd", (True, True, False): "plb_loss_fwd_bwd_dual",
    (True, False, True): "plb_loss_fwd_bwd_packed", (True, True, True): "plb_loss_fwd_bwd_dual_packed",
}


@pytest.mark.parametrize("family, table", [("forward", FORWARD), ("encode", ENCODE)])
def test_forward_and_encode_rungs(family, table):
    for key in itertools.product([False, True], repeat=3):
        assert encoder_entry(family, *key) == table[key], (family, key)


def test_encode_bwd_rungs():
    for inputs, mask, below, want in itertools.product([False, True], repeat=4):
        for layers in (False, True, None):   # what the forward asked for plays no part in the backward's rung
            # (a d_below list whose entries are all None is still the layers rung: the engine reads the list)
            got = encoder_entry("encode_bwd", layers, inputs, mask, [None, None] if below else None, want)
            assert got == ENCODE_BWD[inputs, mask, below, want], (layers, inputs, mask, below, want)


def test_loss_rungs():
    for key in itertools.product([False, True], repeat=3):
        assert loss_entry(*key) == LOSS[key], key


def test_every_reachable_symbol_has_its_arguments_listed():
    reached = set(FORWARD.values()) | set(ENCODE.values()) | set(ENCODE_BWD.values()) | set(LOSS.values()) | {"plb_forward_packed"}
    assert reached == set(ENTRY_ARGS)
    assert set(ENTRY_ARGS) <= set(_lib.PUBLIC)


@pytest.mark.parametrize("name", sorted(ENTRY_ARGS))
def test_argument_names_are_the_headers_in_order(name):
    proto = c_header.public().protos[name]
    assert list(ENTRY_ARGS[name]) == [p.name for p in proto.params]
