"""Every 16-bit GRU recurrence, step by step against float64 (cases, references, restatement and gate in
tests/gru16_cases.py): gru16_fwd / gru16_bwd<H> of csrc/gru16.hip at H = 32, 64, 128, 256 through the lane-native
layout and b2p_gru_lane_permute, and grumc_fwd / grumc_bwd<H> of csrc/grumc.hip at H = 256 (which the dispatcher
never picks), 384, 512 and 1024. Each output of each case obeys

    E_k <= 4 * E_r + 2 * 2^-24 * max|ref64|

with E_k the kernel's largest distance from the float64 step evaluated from the kernel's own previous step and E_r
the same statistic of the fp32 restatement on the same inputs, computed on the host. Every output sits between NaN
guard rows and must be finite under the planted +-20 / +-90 pre-activations; a NaN batch row leaves every other
row bitwise unchanged. b2p_gru_lane_permute and b2p_gru_hprev are held bitwise to index arithmetic."""
import numpy as np
import pytest
import torch

from tests import gru16_cases as gc

pytestmark = pytest.mark.gpu

STEP_CASES = [("gru16", H, *s) for H in gc.H_GRU16 for s in gc.CASES_GRU16] + \
             [("mc", H, *s) for H in gc.H_MC for s in gc.mc_cases(H)]


@pytest.mark.parametrize("backend,H,B,T,nd,has_h0,has_bias", STEP_CASES)
def test_steps_against_float64(backend, H, B, T, nd, has_h0, has_bias):
    c = gc.case(H, B, T, nd, has_h0, has_bias)
    _, got = gc.RUNNERS[backend](c)
    assert (got["dh0"] is None) == (not has_h0)
    ek = gc.errors(c, backend, got)
    er = gc.restate_errors(backend, H, B, T, nd, has_h0, has_bias)
    _, fails = gc.judge(f"{backend} H={H} B={B} T={T} nd={nd} h0={int(has_h0)} bhh={int(has_bias)}", ek, er)
    assert not fails, fails


@pytest.mark.parametrize("backend,H", [("gru16", H) for H in gc.H_GRU16] + [("mc", H) for H in gc.H_MC])
def test_nan_row_stays_in_its_row(backend, H):
    c = gc.case(H, *gc.ISOLATION)
    clean, _ = gc.RUNNERS[backend](c)
    dirty, _ = gc.RUNNERS[backend](c, poison_row=1)
    keep = np.arange(c.B) != 1
    for name in clean:
        a, b = (x[:, keep] if name == "dh0" else x[keep] for x in (clean[name], dirty[name]))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
        assert np.isfinite(a).all(), name


# ---------------------------------------------------------------------------------------- b2p_gru_lane_permute
FILL = -12345.0
# (Rl, Rs, rmap): the four calls of functional.py, and the two 4-record maps into a 4-record standard tensor, whose
# record 3 (to_lane: LN record 3 / 2) no nibble maps
PERMUTES = [(3, 3, 0x210), (1, 1, 0x0), (4, 3, 0xF210), (4, 3, 0x2F10), (4, 4, 0xF210), (4, 4, 0x2F10)]


@pytest.mark.parametrize("H", [32, 256])
@pytest.mark.parametrize("nd", [1, 2])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_lane_permute_bitwise(B, T, H, nd):
    from wav2vec2forbrain_amd import _lib
    g = np.random.default_rng((B, T, H, nd))
    st = _lib.stream_ptr()
    for Rl, Rs, rmap in PERMUTES:
        n_ln, n_std = gc.ln_floats(B, T, H, nd, Rl), B * T * nd * Rs * H
        assert n_ln == int(_lib.load().b2p_gru16_lane_floats(B, T, H, nd, Rl))
        n_pad = -(-B // 16) * 16 * T * nd * Rs * H     # room for the rows b >= B a from-lane call must not write
        for to_lane, n_src, n_dst in ((1, n_std, n_ln), (0, n_ln, n_pad)):
            src = g.standard_normal(n_src).astype(np.float32)
            want = gc.ln_permute(src, np.full(n_dst, FILL, np.float32), B, T, H, nd, Rl, Rs, rmap, to_lane)
            buf = gc.Guarded()
            dst = buf.new(n_dst)
            dst.fill_(FILL)
            srcd = torch.from_numpy(src).cuda()
            _lib.call("b2p_gru_lane_permute", srcd.data_ptr(), dst.data_ptr(), B, T, H, nd, Rl, Rs, rmap, to_lane, st)
            torch.cuda.synchronize()
            buf.check()
            got = dst.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (Rl, Rs, hex(rmap), to_lane)
            mapped = {gc._nib(rmap, k) for k in range(Rl)} - {15}
            if to_lane:      # padded rows are zeros, an unmapped LN record keeps the fill
                assert ((got == 0).any()) == (B % 16 != 0)
                assert ((got == FILL).any()) == any(gc._nib(rmap, k) == 15 for k in range(Rl))
            else:            # rows b >= B and a standard record no nibble maps keep the fill
                assert (got[n_std:] == FILL).all()
                assert ((got[:n_std] == FILL).any()) == (len(mapped) < Rs)


# ----------------------------------------------------------------------------------------------- b2p_gru_hprev
@pytest.mark.parametrize("has_h0", [True, False])
@pytest.mark.parametrize("nd", [1, 2])
@pytest.mark.parametrize("T", [1, 4])
def test_hprev_bitwise(T, nd, has_h0):
    from wav2vec2forbrain_amd import _lib
    B, H = 3, 32
    g = np.random.default_rng((T, nd, int(has_h0)))
    out = g.standard_normal((B, T, nd * H)).astype(np.float32)
    h0 = g.standard_normal((nd, B, H)).astype(np.float32) if has_h0 else None
    want = np.zeros((nd, B, T, H), np.float32)
    for d in range(nd):
        for t in range(T):
            tp = t - 1 if d == 0 else t + 1
            if 0 <= tp < T:
                want[d, :, t] = out[:, tp, d * H:(d + 1) * H]
            elif has_h0:
                want[d, :, t] = h0[d]
    buf = gc.Guarded()
    hp = buf.new(nd * B * T * H)
    h0d = torch.from_numpy(h0).cuda() if has_h0 else None
    outd = torch.from_numpy(out).cuda()
    _lib.call("b2p_gru_hprev", outd.data_ptr(), None if h0d is None else h0d.data_ptr(),
              hp.data_ptr(), B, T, H, nd, _lib.stream_ptr())
    torch.cuda.synchronize()
    buf.check()
    assert np.array_equal(hp.cpu().numpy().view(np.uint32), want.reshape(-1).view(np.uint32))
