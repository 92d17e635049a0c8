"""Which recurrence back-end a GRU layer takes (functional._gru_recurrence / _gru_recurrence_bwd), enumerated
on the host against the table of DESIGN.md section 5: precision mode x bf16x3 forms x switches x hidden size.
No device: the functions read the precision state, the switches and the library's *_supported answers."""
import contextlib

import pytest
import torch

from wav2vec2forbrain_amd import functional as Fn

HS = (32, 48, 64, 128, 256, 384, 512)
POLICY = frozenset({"wgrad", "dgrad2b"})     # the default Trainer policy forms: no GRU form among them
BF16 = {32: "gru16", 64: "gru16", 128: "gru16", 256: "gru16", 384: "mc", 512: "mc", 48: "step"}
MC_SIZES = (256, 384, 512)


@contextlib.contextmanager
def _switch(cell, value):
    """Sets a one-element switch of the module and restores it."""
    old, cell[0] = cell[0], value
    try:
        yield
    finally:
        cell[0] = old


def _bwd_expected(fwd, H, override):
    if fwd == "gru16" or override is None:
        return fwd
    if override and H in MC_SIZES:
        return "mc"
    return "gru32" if fwd == "gru32" else "step"


def _check(H, want):
    """The forward's choice, and the backward's under every _GRUMC_BWD setting."""
    assert Fn._gru_recurrence(H) == want, (H, want)
    for override in (None, True, False):
        with _switch(Fn._GRUMC_BWD, override):
            assert Fn._gru_recurrence_bwd(want, H) == _bwd_expected(want, H, override), (H, want, override)


def test_defaults():
    assert (Fn._GRUMC[0], Fn._GRUMC_BWD[0], Fn._GRU32[0]) == (True, None, True)
    assert not hasattr(Fn, "_GRU16")
    assert Fn.PRECISION_MODES["fp32"] not in Fn.GRU32_MODES and Fn.PRECISION_MODES["bf16x3"] in Fn.GRU32_MODES


@pytest.mark.parametrize("H", HS)
def test_bf16(H):
    with Fn.precision("bf16"):
        _check(H, BF16[H])
        with Fn.persistent_gru32(False):      # not the 16-bit path's switch
            _check(H, BF16[H])
        with _switch(Fn._GRUMC, False):
            _check(H, "step" if H in (384, 512) else BF16[H])


@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("H", HS)
def test_fp32_keeps_the_per_step_kernels(H, on):
    with Fn.precision("fp32"), Fn.persistent_gru32(on):
        _check(H, "step")
        with Fn.x3_forms(["grurec1", "gru1"]):     # the forms belong to the bf16x3 mode only
            _check(H, "step")


@pytest.mark.parametrize("forms", [None, POLICY])
@pytest.mark.parametrize("H", HS)
def test_bf16x3(H, forms):
    with Fn.precision("bf16x3"), Fn.x3_forms(forms):
        _check(H, "gru32" if H in (256, 512) else "step")
        with _switch(Fn._GRUMC, False):     # not the fp32-operand layers' switch
            _check(H, "gru32" if H in (256, 512) else "step")
        with Fn.persistent_gru32(False):
            _check(H, "step")


@pytest.mark.parametrize("H", HS)
def test_bf16x3_grurec1_is_the_16bit_path(H):
    with Fn.precision("bf16x3"), Fn.x3_forms(POLICY | {"grurec1"}), Fn.persistent_gru32(False):
        _check(H, BF16[H])
        with _switch(Fn._GRUMC, False):
            _check(H, "step" if H in (384, 512) else BF16[H])


@pytest.mark.parametrize("H", HS)
def test_bf16x3_gru1_wrapping_of_gru_layer(H, monkeypatch):
    """gru_layer runs a 'gru1' layer under precision('bf16'): the choice made inside it is bf16's."""
    monkeypatch.setattr(Fn._GRULayer, "apply", lambda x, unf, H, ndir, h0, *w: Fn._gru_recurrence(H))
    x = torch.zeros(1, 1, 8)
    with Fn.precision("bf16x3"), Fn.x3_forms(POLICY | {"gru1"}):
        assert Fn.gru_layer(x, H, 1, []) == BF16[H]
        assert Fn.gru_layer(Fn.Unfolded(x, 1, 1), H, 1, []) == BF16[H]
    with Fn.precision("bf16x3"), Fn.x3_forms(POLICY):
        assert Fn.gru_layer(x, H, 1, []) == ("gru32" if H in (256, 512) else "step")


def test_status_kinds_come_from_the_table():
    kinds = {k for be in Fn._GRU_BACKENDS.values() for k in be.kinds if k}
    assert kinds == {1, 2, 3, 4} and Fn._GRU_BACKENDS["step"].kinds == (None, None)
    for kind, text in ((1, "(forward of"), (2, "(backward of"), (3, "(exact-fp32 forward of"), (4, "(exact-fp32 backward of")):
        assert text in str(Fn._gru_status_error(kind * 65536 + 3))
