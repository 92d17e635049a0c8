"""The multi-CU persistent GRU recurrence at hidden size 1024 (csrc/grumc.hip), host side: the shape class, the
workspace layout, which back-end a layer of H = 1024 takes under every mode and switch and
the status word's size code. No device: the functions read the precision state, the switches and the library's
answers (the pattern of tests/test_gru_dispatch_host.py)."""
import contextlib

import pytest

from wav2vec2forbrain_amd import _lib
from wav2vec2forbrain_amd import functional as Fn

POLICY = frozenset({"wgrad", "dgrad2b"})     # the default Trainer policy forms: no GRU form among them


@contextlib.contextmanager
def _switch(cell, value):
    old, cell[0] = cell[0], value
    try:
        yield
    finally:
        cell[0] = old


def _groups(B, nd):
    return nd * ((B + 15) // 16)


def _ws1024(B, nd):
    """The documented H = 1024 layout (include/b2p_hip.h): 16 B of fail words, 16 member ids of 8 B per
    recurrence, then per recurrence 2 slots of 16 members x 1024 granules of 8 B."""
    g = _groups(B, nd)
    return 16 + g * 16 * 8 + g * 2 * 16 * 1024 * 8


def test_supported_sizes():
    lib = _lib.load()
    for H in (256, 384, 512, 1024):
        assert lib.b2p_gru_mc_supported(H) == 1, H
    for H in (768, 2048, 0, 64, 1023, 1088):
        assert lib.b2p_gru_mc_supported(H) == 0, H


@pytest.mark.parametrize("B,nd", [(1, 1), (16, 2), (65, 2), (129, 2)])
def test_workspace_1024_layout(B, nd):
    ws = int(_lib.load().b2p_gru_mc_workspace(B, 1024, nd))
    assert ws > 0 and ws % 16 == 0
    assert ws == _ws1024(B, nd)


def test_workspace_1024_monotone_in_batch():
    lib = _lib.load()
    for nd in (1, 2):
        sizes = [int(lib.b2p_gru_mc_workspace(B, 1024, nd)) for B in range(1, 300)]
        assert all(s > 0 and s % 16 == 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))
        assert sizes[15] < sizes[16]      # B = 16 -> 17: one more batch group


@pytest.mark.parametrize("B,nd", [(1, 1), (16, 2), (17, 1), (65, 2), (129, 2)])
def test_workspace_512_keeps_its_formula(B, nd):
    want = 16 + 32 * 16 * 8 + nd * ((B + 15) // 16) * 2 * 8 * 1024 * 8
    assert int(_lib.load().b2p_gru_mc_workspace(B, 512, nd)) == want
    assert int(_lib.load().b2p_gru_mc_workspace(B, 768, nd)) == 0


def _check(want):
    assert Fn._gru_recurrence(1024) == want
    for override, bwd in ((None, want), (True, "mc"), (False, "step")):
        with _switch(Fn._GRUMC_BWD, override):
            assert Fn._gru_recurrence_bwd(want, 1024) == bwd, (want, override)


@pytest.mark.parametrize("g32", [True, False])
def test_recurrence_choice_at_1024(g32):
    with Fn.persistent_gru32(g32):       # the fp32-operand layers' switch changes nothing at this size
        with Fn.precision("bf16"):
            _check("mc")
            with _switch(Fn._GRUMC, False):
                _check("step")
        with Fn.precision("bf16x3"), Fn.x3_forms(POLICY | {"grurec1"}):
            _check("mc")
            with _switch(Fn._GRUMC, False):
                _check("step")
        for forms in (None, POLICY):
            with Fn.precision("bf16x3"), Fn.x3_forms(forms):
                _check("step")           # csrc/gru32.hip has no H = 1024
        with Fn.precision("fp32"):
            _check("step")
            with Fn.x3_forms(["grurec1", "gru1"]):
                _check("step")


def test_no_scratch_in_any_instantiation():
    """A W_hh fragment spilled to scratch would be re-read from memory every step: every grumc kernel, the
    H = 1024 ones included, compiles to 0 bytes of scratch per lane (the compiler's own resource listing)."""
    from wav2vec2forbrain_amd import build_lib
    scratch = {k: v for k, v in build_lib.audit_scratch("grumc.hip").items() if "grumc_" in k}
    for kind in ("fwd", "bwd"):
        for H in (256, 384, 512, 1024):
            hit = [k for k in scratch if f"grumc_{kind}ILi{H}E" in k]
            assert len(hit) == 1, (kind, H, sorted(scratch))
            assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])


def test_status_error_names_the_size():
    assert "H=1024" in str(Fn._gru_status_error(1 * 65536 + 4))
    assert "(forward of" in str(Fn._gru_status_error(1 * 65536 + 4))
    assert "(backward of" in str(Fn._gru_status_error(2 * 65536 + 7 * 16 + 4))
    assert "layer 7, H=1024" in str(Fn._gru_status_error(2 * 65536 + 7 * 16 + 4))
    assert "H=512" in str(Fn._gru_status_error(1 * 65536 + 3))
    assert "H=384" in str(Fn._gru_status_error(1 * 65536 + 2))
    assert "H=256" in str(Fn._gru_status_error(1 * 65536 + 1))
