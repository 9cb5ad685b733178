"""Gradient accumulation and clipping, host side (no GPU): the size of the norm buffer and every misuse of
plb_grad_accum_add / plb_grad_norm / plb_adamw_step_clipped that can be reached on an engine with no device memory bound.
Each must return non-zero BEFORE anything is launched, with a text that says what is wrong. (The one misuse that needs a
backward call to set up — micro-steps of one window on different parameters — is in tests/test_gpu_grad_accum.py.)"""
import ctypes as C

import pytest

from plbert_amd import _lib


@pytest.fixture
def engine():
    L = _lib.lib()
    c = _lib.PlbConfig(188, 64, 128, 2, 256, 2, 512, 2, 1e-12, 188, 8, 4, 32, 0)
    h = C.c_void_p()
    assert L.plb_create(C.byref(c), C.byref(h)) == 0
    yield L, h
    L.plb_destroy(h)


def _err(L):
    return L.plb_last_error().decode()


def test_norm_buffer_size_covers_results_and_two_sets_of_partials(engine):
    L, h = engine
    assert _lib.PLB_NORM_PARTS == 1024
    assert L.plb_grad_norm_floats(h) >= 4 + _lib.PLB_NORM_PARTS * 2
    assert L.plb_grad_norm_floats(None) < 0
    # the chunk a workgroup owns and the addition chain behind its partial (csrc/plbert_kernels.h), as the tests use them
    assert [_lib.norm_chunk(n) for n in (4, 1024, 1028, 1024 * 1024, 1024 * 1024 + 4)] == [1024, 1024, 1024, 1024, 2048]
    assert _lib.norm_chain(4) == 4 + 6 + 3 and _lib.norm_chain(1024 * 1024 + 4) == 8 + 6 + 3


def test_accumulation_misuse_fails_with_a_text_before_anything_is_launched(engine):
    L, h = engine
    fake = C.c_void_p(1 << 20)    # never dereferenced: every call below fails on host state alone
    # no buffer bound
    for phase in (0, 1, 2):
        assert L.plb_grad_accum_add(h, phase, None, None) != 0
        assert "no accumulation buffer bound" in _err(L)
    assert L.plb_grad_accum_bind(h, C.c_void_p((1 << 20) + 4)) != 0 and "16-byte aligned" in _err(L)
    assert L.plb_grad_accum_bind(h, fake) == 0
    # ADD or LAST without a FIRST
    for phase in (1, 2):
        assert L.plb_grad_accum_add(h, phase, None, None) != 0
        assert "without a FIRST" in _err(L) and "no window is open" in _err(L)
    # nothing new in the gradient buffer: no backward entry point has run (the state an add leaves behind as well)
    assert L.plb_grad_accum_add(h, 0, None, None) != 0
    assert "added twice" in _err(L)
    # a phase that does not exist; partial sums anywhere but at LAST
    assert L.plb_grad_accum_add(h, 3, None, None) != 0 and "phase 3" in _err(L)
    assert L.plb_grad_accum_add(h, 0, fake, None) != 0 and "LAST" in _err(L)
    # unbinding brings the first text back
    assert L.plb_grad_accum_bind(h, None) == 0
    assert L.plb_grad_accum_add(h, 0, None, None) != 0 and "no accumulation buffer bound" in _err(L)


def test_norm_and_clipped_update_misuse(engine):
    L, h = engine
    fake = C.c_void_p(1 << 20)
    assert L.plb_grad_norm(h, 1.0, 1.0, None, 0, None) != 0 and "norm_buf" in _err(L)
    assert L.plb_grad_norm(h, 1.0, 1.0, fake, 1, None) != 0 and "left none in this buffer" in _err(L)
    assert L.plb_grad_norm(h, 1.0, 1.0, fake, 0, None) != 0 and "not bound" in _err(L)
    assert L.plb_adamw_step_clipped(h, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 1.0, fake, None) != 0 and "not bound" in _err(L)
    assert L.plb_grad_norm(None, 1.0, 1.0, fake, 0, None) != 0 and "null engine" in _err(L)
