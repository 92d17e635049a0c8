"""The long class of the fused exact-fp32 attention (csrc/attn32.hip: b2p_attn32_long_fwd / _bwd, 257 <= T' <=
512) on the device. The form and the rule are tests/test_attn32_gpu.py's:

Every kernel case uses head size 64, B = 2, heads = 2 (batch and head strides both exercised), qkv = randn * 0.5
and dO = randn from a generator seeded 1000 + T', and is held against a float64 restatement on the CPU with a
bound MEASURED in the same test from the unfused path (functional._attn_core_fwd / _bwd under
fused_attn32(False) in fp32 mode):

    E_f <= 2 * E_u + 4 * 2**-24 * max|ref|     (max abs errors against float64, per output)

Both forms are fp32 sums of the same lengths that differ in order (here also in the two-chunk online softmax and
its rescaling by exp2(m_old - m_new)) and in the exp form; a factor 2 plus 4 ulp of the output scale absorbs
that, while any 16-bit rounding inside the kernel would be ~10^3 times larger. The unfused path produces no lse,
so lse2 (checked as ln: lse2 * ln 2) is held to the 4-ulp term alone (E_u = 0): it is one fp32 value whose own
rounding, at most half an ulp of max|ref| / ln 2 in the log2 domain, plus one v_log_f32 result and one fused
multiply-add, stays below 4 ulp of max|ref|.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.attn32_cases import Attn32Cases, attn_gemms as _attn_gemms, batch as _batch, fn as _fn, \
    nan_bufs as _nan_bufs, ref64_plain as _ref64, three_steps, unfused as _unfused
from tests.helpers import CFG, load_fixture, build_model

pytestmark = pytest.mark.gpu

_CASES = Attn32Cases("b2p_attn32_long_fwd", "b2p_attn32_long_bwd", "attn32_long")
_fused, _hold, _dropout_case = _CASES.fused, _CASES.hold, _CASES.dropout_case


@pytest.mark.timeout(120)
@pytest.mark.parametrize("T", [257, 273, 313, 384, 385, 511, 512])
def test_against_float64(T):
    """O, lse2 and dqkv without dropout: one key in the second chunk and one query in the third 128-block, a
    tile edge past the chunk edge, the base_L1280 fixture's T', the 128-block edge inside the second chunk from
    both sides, the odd T' where TP != T', and the limit."""
    Oref, lse_ref, dref = _ref64(T)
    O, lse2, dqkv, _ = _fused(T, 0.0)
    Ou, du, _, _ = _unfused(T, 0.0)
    res = [_hold("O", T, O, Ou, Oref), _hold("dqkv", T, dqkv, du, dref),
           _hold("lse", T, lse2.double() * math.log(2.0), None, lse_ref)]
    assert all(ok for ok, _ in res), [r for ok, r in res if not ok]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("T", [257, 313, 511])
def test_dropout_identity(T, p):
    """The long kernels draw the unfused softmax kernel's keep mask element for element (forward and both
    backward kernels' rehash, in both chunks), eagerly and under a seed epoch with the counter at 3."""
    Fn = _fn()
    lib = Fn._lib.load()
    O0 = _dropout_case(T, p)
    ctr = torch.full((1,), 3, dtype=torch.int64, device="cuda")
    try:
        Fn._lib.check(lib.b2p_set_seed_epoch(ctypes.c_void_p(ctr.data_ptr())), "set_seed_epoch")
        O3 = _dropout_case(T, p)
        ctr.zero_()
        Oz = _fused(T, p)[0]
    finally:
        Fn._lib.check(lib.b2p_set_seed_epoch(None), "set_seed_epoch")
    assert torch.equal(Oz, O0)          # counter 0 = the eager mask
    assert not torch.equal(O3, O0)      # counter 3 draws another


@pytest.mark.timeout(120)
def test_every_element_written_once_and_bitwise_repeatable():
    T, p = 385, 0.1
    a = _fused(T, p, bufs=_nan_bufs(T))
    for t in a:
        assert not bool(torch.isnan(t).any())
    b = _fused(T, p, bufs=_nan_bufs(T))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.timeout(120)
def test_layerdrop_gate():
    """Gate flag 1: the ungated bits. Flag 0: O = 0, a finite lse2, zeros over dqkv and delta_ws."""
    Fn = _fn()
    T, p = 385, 0.1
    base = _fused(T, p)
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    try:
        Fn._lib.call("b2p_set_gate", flag.data_ptr())
        opened = _fused(T, p, bufs=_nan_bufs(T))
        flag.zero_()
        closed = _fused(T, p, bufs=_nan_bufs(T))
    finally:
        Fn._lib.call("b2p_set_gate", None)
    for x, y in zip(base, opened):
        assert torch.equal(x, y)
    O, lse2, dqkv, delta = closed
    assert bool((O == 0).all()) and bool(torch.isfinite(lse2).all())
    assert bool((dqkv == 0).all()) and bool((delta == 0).all())


# the tiny Conformer with head size 64 and 1,280-bin windows: T' = 313, as base_L1280
CONF_LONG = dict(CFG["tiny_conf"], name="tiny_conf_h64_L1280", hidden_size=128, heads=2, L=1280, in_lens=[1280, 1100])


def _fused_and_unfused(cfg, mode):
    """{fused: (loss, batched attention GEMMs logged, parameter gradients)} of one forward + backward each."""
    Fn = _fn()
    model = build_model(cfg)
    model.train()
    batch = _batch(cfg)
    nz = cfg["B"] * cfg["heads"]
    assert Fn.ATTN32_MODES == (3,)
    runs = {}
    for fused in (False, True):
        for prm in model.parameters():
            prm.grad = None
        Fn.GEMM_LOG = []
        try:
            if mode == "fp32":      # the fp32 mode's default keeps the unfused path: its fused run is selected here
                Fn.ATTN32_MODES = (1, 3)
            with Fn.precision(mode), Fn.fused_attn32(fused):
                out = model(batch)
                out.loss.backward()
            torch.cuda.synchronize()
            log = Fn.GEMM_LOG
        finally:
            Fn.GEMM_LOG = None
            Fn.ATTN32_MODES = (3,)
        runs[fused] = (float(out.metrics["ctc_loss"]), _attn_gemms(log, nz),
                       {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None})
    return runs


def _hold_fused_against_unfused(cfg, mode, runs, gmax):
    (lu, gu, du), (lf, gf, df) = runs[False], runs[True]
    assert len(gu) == 6 * cfg["layers"], (mode, len(gu))
    Ts = {e["M"] for e in gu}
    assert len(Ts) == 1 and 256 < max(Ts) <= 512, Ts
    assert gf == [], (mode, len(gf))        # fused: no batched attention GEMM is left
    assert set(df) == set(du)
    for n, g in du.items():
        tol = 2e-3 * max(float(g.abs().max()), 1e-3 * gmax)
        assert float((df[n] - g).abs().max()) <= tol, (mode, n)
    return max(Ts), lf, lu


@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_base_L1280_takes_the_fused_path_and_matches_its_golden(mode):
    """The numbers of test_attn32_gpu.py::test_models_take_the_fused_path_and_match_goldens on the post-LN base
    model with 1,280-bin windows (12 layers, T' = 313)."""
    cfg = CFG["base_L1280"]
    fx = load_fixture("base_L1280")
    ref = float(fx["loss"])
    gmax = max(float(fx["gnorm/" + n]) for n in fx["param_names"])
    assert cfg["hidden_size"] // cfg["heads"] == 64
    Tq, lf, lu = _hold_fused_against_unfused(cfg, mode, _fused_and_unfused(cfg, mode), gmax)
    print(f"base_L1280 [{mode}]: T' {Tq} loss fused {lf:.9g} unfused {lu:.9g} golden {ref:.9g}")
    assert Tq == 313
    if mode == "fp32":
        assert abs(lf - ref) <= 2e-5 * abs(ref), (lf, ref)
    else:
        assert abs(lf - ref) <= abs(lu - ref) + 2e-5 * abs(ref), (lf, lu, ref)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_conformer_takes_the_fused_path(mode):
    """The Conformer's rotary attention core at T' = 313 (no golden at this length): fused against unfused, the
    same gradient rule with the unfused run's largest gradient norm in the fixture's place."""
    runs = _fused_and_unfused(CONF_LONG, mode)
    gmax = max(float(g.norm()) for g in runs[False][2].values())
    Tq, lf, lu = _hold_fused_against_unfused(CONF_LONG, mode, runs, gmax)
    print(f"{CONF_LONG['name']} [{mode}]: T' {Tq} loss fused {lf:.9g} unfused {lu:.9g}")
    assert np.isfinite(lf) and np.isfinite(lu), (lf, lu)


def _three_steps(graphs):
    """attn32_cases.three_steps at T' = 313, as test_attn32_gpu.py runs it at T' <= 256."""
    return three_steps(CONF_LONG, graphs)


@pytest.mark.timeout(300)
def test_captured_steps_match_eager_steps_with_the_same_draws():
    """A captured step replays the long kernels with each replay's own dropout masks (the seed epoch) and
    LayerDrop gates: one eager step, the capture and two replays give the losses and parameters of eager steps
    with the same draws, in the form and tolerance of test_attn32_gpu.py's test of the same name."""
    le, pe, ne, pate = _three_steps(False)
    lg, pg, ng, patg = _three_steps(True)
    print(f"captured steps: losses replayed {lg} eager {le}, LayerDrop keep patterns {patg}")
    assert ne == 0 and ng == 0, (ne, ng)     # no batched attention GEMM: the long kernels ran
    assert patg == pate and len(patg) == 2
    assert all(np.isfinite(lg))
    np.testing.assert_allclose(lg, le, rtol=1e-5, atol=0)
    for n in pe:
        assert float((pg[n] - pe[n]).norm()) <= 1e-5 * float(pe[n].norm()) + 1e-7, n
