"""The activation table off the device: the tests' float64 restatement pinned to transformers'
ACT2FN, every name of the ACTIVATION_FUNCTION literal reachable from the arguments down to an id,
and the C ABI's rejection of ids outside the table (no launch, so no device is needed)."""
import ctypes
import typing

import numpy as np
import pytest
import torch

from tests import act_cases as AC


def test_restatement_matches_transformers():
    """Every name's float64 restatement equals ACT2FN[name] on the kernel tests' grid to 1e-12 (of
    max(1, |value|): relu2(1e30) is 1e60)."""
    tf = pytest.importorskip("transformers.activations")
    x = AC.grid().double()
    for name in AC.NAMES:
        want = tf.ACT2FN[name](x)
        got = AC.FN[name](x)
        err = float(((got - want).abs() / want.abs().clamp_min(1.0)).max())
        assert err <= 1e-12, (name, err)


def test_tanh_gelu_spellings_are_one_function():
    """gelu_new / gelu_fast / gelu_pytorch_tanh / gelu_accurate share B2P_ACT_GELU_TANH: their values
    and derivatives differ from the id's formula by far less than the kernels' fp32 bound."""
    x = AC.grid()
    v0, g0 = AC.truth(AC.ID_NAME[AC.IDS["gelu_new"]], x)
    for name in AC.TANH_GELU_NAMES:
        assert AC.IDS[name] == AC.IDS["gelu_new"]
        v, g = AC.truth(name, x)
        ev = float(((v - v0).abs() / v0.abs().clamp_min(1.0)).max())
        eg = float(((g - g0).abs() / g0.abs().clamp_min(1.0)).max())
        print(f"{name}: value {ev:.2e} derivative {eg:.2e} (fp32 bound {AC.BOUND:.2e})")
        assert ev <= 1e-3 * AC.BOUND and eg <= 1e-3 * AC.BOUND, (name, ev, eg)


def test_grid_keeps_clear_of_kinks():
    x = AC.grid()
    assert x.dtype == torch.float32 and x.numel() == 1034
    for k in AC.KINKS:
        assert float((x.double() - k).abs().min()) > 1e-3


def test_literal_is_covered():
    from wav2vec2forbrain_amd import functional as Fn
    from wav2vec2forbrain_amd.util import nn_helper
    names = typing.get_args(nn_helper.ACTIVATION_FUNCTION)
    assert sorted(names) == AC.NAMES and len(names) == 18
    for n in names:
        assert n in nn_helper.SUPPORTED_ACTIVATIONS, n
        assert Fn.ACT[n] == AC.IDS[n], n
        assert Fn.ACT[nn_helper.SUPPORTED_ACTIVATIONS[n]] == AC.IDS[n], n
    assert Fn.EPILOGUE_ACTS == {0, 1, 2, 3}
    assert max(Fn.ACT.values()) == AC.ID_LAST


def test_header_ids():
    """The ids of include/b2p_hip.h are the ones the tests and functional.ACT use; 0-3 keep their values."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "b2p_hip.h")).read()
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"B2P_ACT_([A-Z0-9_]+) = (\d+)", src)}
    assert ids == {"none": 0, "gelu": 1, "softsign": 2, "silu": 3, "gelu_tanh": 4, "gelu_10": 5, "quick_gelu": 6,
                   "laplace": 7, "mish": 8, "relu": 9, "relu2": 10, "relu6": 11, "sigmoid": 12, "tanh": 13}


@pytest.mark.parametrize("name", AC.NAMES)
def test_create_fully_connected_builds(name):
    from wav2vec2forbrain_amd import functional as Fn
    from wav2vec2forbrain_amd.util.nn_helper import Activation, create_fully_connected
    fc = create_fully_connected(32, 48, [40], name)
    mods = list(fc)
    assert [type(m).__name__ for m in mods] == ["Linear", "Activation", "Linear"]
    assert isinstance(mods[1], Activation) and Fn.ACT[mods[1].name] == AC.IDS[name]


def test_args_model_accepts_a_table_activation():
    from wav2vec2forbrain_amd.model.brain_feature_extractor import B2P2TBrainFeatureExtractorArgsModel
    a = B2P2TBrainFeatureExtractorArgsModel(encoder_fc_activation_function="relu", encoder_fc_hidden_sizes=[40])
    assert a.encoder_fc_activation_function == "relu" and a.encoder_fc_hidden_sizes == [40]


def test_workload_selects_the_activation():
    from wav2vec2forbrain_amd.util.nn_helper import Activation
    from wav2vec2forbrain_amd.workloads import build_model, tiny_act_config
    for name, want in (("mish", "mish"), ("gelu_fast", "gelu_new")):
        m = build_model(tiny_act_config(name), device="cpu")
        acts = [x for x in m.modules() if isinstance(x, Activation)]
        assert [a.name for a in acts] == [want]
    cfg = tiny_act_config()
    del cfg["fc_activation"]   # a workload without the key keeps gelu
    assert [x.name for x in build_model(cfg, device="cpu").modules() if isinstance(x, Activation)] == ["gelu"]


def test_functional_gemm_rejects_a_table_activation():
    from wav2vec2forbrain_amd import functional as Fn
    with pytest.raises(ValueError, match="relu"):
        Fn.gemm(4, 4, 4, None, None, None, 4, act=Fn.ACT["relu"])
    with pytest.raises(ValueError, match="mish"):
        Fn.gemm(4, 4, 4, None, None, None, 4, act_bwd=Fn.ACT["mish"])


def test_c_abi_rejects_ids_outside_the_table():
    from wav2vec2forbrain_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "b2p_act_fwd") and "b2p_act_fwd" in _lib.exported_symbols()
    buf = np.zeros(8, dtype=np.float32)
    p = buf.ctypes.data
    for bad in (99, -1, AC.ID_LAST + 1):
        assert lib.b2p_act_fwd(p, p, 8, bad, None) != 0
        assert str(bad).encode() in lib.b2p_last_error() and b"act_fwd" in lib.b2p_last_error()
        assert lib.b2p_act_bwd(p, p, p, 8, bad, None) != 0
        assert str(bad).encode() in lib.b2p_last_error() and b"act_bwd" in lib.b2p_last_error()
    with pytest.raises(RuntimeError, match="99"):
        _lib.call("b2p_act_fwd", p, p, 8, 99, None)
    # n = 0 with a valid id: nothing to launch
    assert lib.b2p_act_fwd(p, p, 0, AC.ID_LAST, None) == 0
    assert lib.b2p_act_bwd(p, p, p, 0, AC.ID_LAST, None) == 0


def test_gemm_and_cast_reject_non_epilogue_ids():
    """The epilogues know ids 0-3; any other id is an error that points at b2p_act_fwd, not identity."""
    from wav2vec2forbrain_amd import _lib
    lib = _lib.load()
    for field in ("act", "act_bwd"):
        for bad in (AC.IDS["relu"], 99, -2):
            d = _lib.GemmDesc()
            d.M, d.N, d.K, d.nz1, d.nz2 = 4, 4, 4, 1, 1
            setattr(d.ep, field, bad)
            assert lib.b2p_gemm(ctypes.byref(d), None) != 0
            msg = lib.b2p_last_error()
            assert b"b2p_act_fwd" in msg and str(bad).encode() in msg, msg
    buf = np.zeros(8, dtype=np.float32)
    assert lib.b2p_act_dropout_cast16(buf.ctypes.data, buf.ctypes.data, 8, AC.IDS["relu"], 0.0, 0, None) != 0
    assert b"b2p_act_fwd" in lib.b2p_last_error()
