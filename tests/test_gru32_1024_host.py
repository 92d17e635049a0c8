"""The persistent exact-fp32 GRU recurrence at hidden size 1024 (csrc/gru32.hip), host side: which back-end a
layer takes with the bf16x3 mode's 'gru32w' form, that the form changes nothing anywhere
else, that the Trainer's default policy carries it, and that no gru32 kernel spills. No device."""
import contextlib
import os
import subprocess
import sys

import pytest

from wav2vec2forbrain_amd import functional as Fn

POLICY = frozenset({"wgrad", "dgrad2b"})     # the GEMM forms of the Trainer policy
WIDE = POLICY | {"gru32w"}


@contextlib.contextmanager
def _switch(cell, value):
    old = cell[0]
    cell[0] = value
    try:
        yield
    finally:
        cell[0] = old


def test_form_selects_gru32_at_1024():
    with Fn.precision("bf16x3"), Fn.x3_forms(WIDE):
        assert Fn._gru_recurrence(1024) == "gru32"
        with Fn.persistent_gru32(False):
            assert Fn._gru_recurrence(1024) == "step"
        # the backward follows the forward; the diagnostic re-routes it
        assert Fn._gru_recurrence_bwd("gru32", 1024) == "gru32"
        with _switch(Fn._GRUMC_BWD, True):
            assert Fn._gru_recurrence_bwd("gru32", 1024) == "mc"
        with _switch(Fn._GRUMC_BWD, False):
            assert Fn._gru_recurrence_bwd("gru32", 1024) == "gru32"


@pytest.mark.parametrize("H", [32, 64, 128, 256, 384, 512])
def test_form_changes_nothing_below_1024(H):
    for g32 in (True, False):
        with Fn.persistent_gru32(g32):
            for mode in ("bf16x3", "fp32", "bf16"):
                with Fn.precision(mode):
                    with Fn.x3_forms(POLICY):
                        want = Fn._gru_recurrence(H)
                    with Fn.x3_forms(WIDE):
                        assert Fn._gru_recurrence(H) == want, (H, mode, g32)
    with Fn.precision("bf16x3"), Fn.x3_forms(WIDE):
        assert Fn._gru_recurrence(H) == ("gru32" if H in (256, 512) else "step")


def test_form_changes_nothing_in_other_modes_or_with_grurec1():
    with Fn.precision("fp32"), Fn.x3_forms(WIDE):
        assert Fn._gru_recurrence(1024) == "step"
    with Fn.precision("bf16"), Fn.x3_forms(WIDE):
        assert Fn._gru_recurrence(1024) == "mc"
    with Fn.precision("bf16x3"), Fn.x3_forms(WIDE | {"grurec1"}):
        assert Fn._gru_recurrence(1024) == "mc"      # the 16-bit path goes first
    with Fn.precision("bf16x3"), Fn.x3_forms(None):
        assert Fn._gru_recurrence(1024) == "step"
    assert Fn.x3_mfma_work(WIDE) == Fn.x3_mfma_work(POLICY)   # no GEMM role


def test_default_policy_contains_the_form():
    """With B2P_X3_POLICY unset the Trainer policy's forms are the two GEMM forms and 'gru32w'; 'none' selects
    nothing (a fresh interpreter each: the variable is read at import)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from wav2vec2forbrain_amd import functional as Fn; print(','.join(sorted(Fn.X3_POLICY_FORMS)))"
    for value, want in ((None, "dgrad2b,gru32w,wgrad"), ("none", "")):
        env = {k: v for k, v in os.environ.items() if k != "B2P_X3_POLICY"}
        if value is not None:
            env["B2P_X3_POLICY"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.strip().splitlines()
        assert (lines[-1] if lines else "") == want, r.stdout


def test_no_scratch_in_any_instantiation():
    """A W_hh value spilled to scratch would be re-read from memory every step: every gru32 kernel, the H = 1024
    ones included, compiles to 0 bytes of scratch per lane (the compiler's own resource listing)."""
    from wav2vec2forbrain_amd import build_lib
    scratch = {k: v for k, v in build_lib.audit_scratch("gru32.hip").items() if "gru32_" in k}
    for kind in ("fwd", "bwd"):
        for H in (256, 512, 1024):
            hit = [k for k in scratch if f"gru32_{kind}ILi{H}E" in k]
            assert len(hit) == 1, (kind, H, sorted(scratch))
            assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
