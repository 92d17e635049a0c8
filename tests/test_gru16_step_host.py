"""Host checks of what tests/test_gru16_step_gpu.py relies on (tests/gru16_cases.py); no GPU.

1. The two restatements of the lane-native layout agree: the plain loops written from the header comment of
   csrc/gru16.hip and the vectorised form the GPU module compares b2p_gru_lane_permute against.
2. ref_fwd64 / ref_bwd64 fed with restate32's outputs reproduce a plain free-running float64 GRU whose recurrent
   product rounds the same operands (fp16 h and W_hh forward; bf16 dgh and W_hh in its hand-written backward) and
   whose gradients otherwise come from autograd. The shapes are ones where the 16-bit images of the two runs are
   equal (asserted), so the references see the same operands and differ from the free run only through the fp32 h / saved
   values they are fed: by at most T * E_r(h) in h, nothing in r, z, n, ghn, and 32 (T + 1) max E_r in the backward
   (products of at most four factors, each perturbed by at most (T + 1) E_r, their magnitudes below 32).
3. The gate discriminates: for every back-end and hidden size, each planted defect pushes at least one output past
   the gate by a factor of 10 or more (a condition, not a measurement)."""
import numpy as np
import pytest
import torch

from tests import gru16_cases as gc

LN_SHAPES = [(1, 1, 32, 1), (17, 3, 32, 2), (15, 2, 64, 2)]            # (B, T, H, ndir)
LN_MAPS = [(3, 3, 0x210), (1, 1, 0x0), (4, 3, 0xF210), (4, 3, 0x2F10), (4, 4, 0xF210), (4, 4, 0x3210)]


@pytest.mark.parametrize("B,T,H,nd", LN_SHAPES)
def test_ln_restatements_agree(B, T, H, nd):
    g = np.random.default_rng(B + T + H)
    for Rl, Rs, rmap in LN_MAPS:
        stdv = g.standard_normal(B * T * nd * Rs * H).astype(np.float32)
        lnv = g.standard_normal(gc.ln_floats(B, T, H, nd, Rl)).astype(np.float32)
        for to_lane, src, n_dst in ((1, stdv, lnv.size), (0, lnv, stdv.size)):
            a = gc.ln_permute_loops(src, np.full(n_dst, -7.5, np.float32), B, T, H, nd, Rl, Rs, rmap, to_lane)
            b = gc.ln_permute(src, np.full(n_dst, -7.5, np.float32), B, T, H, nd, Rl, Rs, rmap, to_lane)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (Rl, Rs, hex(rmap), to_lane)
            if to_lane and (rmap >> (4 * (Rl - 1))) & 15 == 15:
                assert (a == -7.5).any()          # the unmapped LN record keeps the fill
    # a round trip through the lane-native layout is the identity
    x = g.standard_normal(B * T * nd * 3 * H).astype(np.float32)
    ln = gc.ln_permute(x, np.zeros(gc.ln_floats(B, T, H, nd, 3), np.float32), B, T, H, nd, 3, 3, 0x210, 1)
    assert np.array_equal(gc.ln_permute(ln, np.zeros_like(x), B, T, H, nd, 3, 3, 0x210, 0), x)


def test_proc_std_round_trip():
    x = np.random.default_rng(0).standard_normal((3, 4, 2 * 3 * 16)).astype(np.float32)
    p = gc.proc(x, 2, 3)
    assert np.array_equal(p[1, 0, 2, 1], x[2, 3, 4 * 16:5 * 16]) and np.array_equal(gc.std(p), x)


class _Rec(torch.autograd.Function):
    """gh = fp16(h) fp16(W)^T in float64; backward dh = bf16(dgh) bf16(W): the operands the kernels round."""
    images = None

    @staticmethod
    def forward(ctx, h, W, key):
        ctx.W, ctx.key = W, key
        h16 = gc.r16(h.detach().numpy().astype(np.float32))
        _Rec.images["h"][key] = h16
        return torch.from_numpy(h16.astype(np.float64)) @ torch.from_numpy(gc.r16(W.numpy()).astype(np.float64)).t()

    @staticmethod
    def backward(ctx, g):
        g16 = gc.rbf(g.numpy().astype(np.float32))
        _Rec.images["dgh"][ctx.key] = g16
        return torch.from_numpy(g16.astype(np.float64)) @ torch.from_numpy(gc.rbf(ctx.W.numpy()).astype(np.float64)), None, None


def _free64(c, backend):
    """The free-running float64 GRU: processing-order h, r, z, n, ghn, dgi, dgh, dh0 and the 16-bit images."""
    nd, T, B, H = c.nd, c.T, c.B, c.H
    gi_p, bias, do = gc._terms(c, backend)
    gi = torch.from_numpy(gi_p.astype(np.float64)).requires_grad_(True)
    h0 = torch.zeros(nd, B, H, dtype=torch.float64) if c.h0 is None else torch.from_numpy(c.h0.astype(np.float64))
    h0.requires_grad_(True)
    _Rec.images = {"h": {}, "dgh": {}}
    hs, ghs, sv = [], [], {k: [] for k in "rzng"}
    for d in range(nd):
        h = h0[d]
        W = torch.from_numpy(np.array(c.whh[d]))
        for s in range(T):
            gh = _Rec.apply(h, W, (d, s)).view(B, 3, H) + torch.from_numpy(bias[d].astype(np.float64))
            gh.retain_grad()
            r = torch.sigmoid(gi[d, s, :, 0] + gh[:, 0])
            z = torch.sigmoid(gi[d, s, :, 1] + gh[:, 1])
            n = torch.tanh(gi[d, s, :, 2] + r * gh[:, 2])
            h = (1 - z) * n + z * h
            hs.append(h)
            ghs.append(gh)
            for k, v in zip("rzng", (r, z, n, gh[:, 2])):
                sv[k].append(v.detach().numpy())
    out = torch.stack(hs).view(nd, T, B, H)
    out.backward(torch.from_numpy(do.astype(np.float64)))
    shp = lambda l, *s: np.stack(l).reshape(nd, T, *s)
    res = {"h": out.detach().numpy(), "r": shp(sv["r"], B, H), "z": shp(sv["z"], B, H), "n": shp(sv["n"], B, H),
           "ghn": shp(sv["g"], B, H), "dgi": gi.grad.numpy(), "dgh": shp([g.grad.numpy() for g in ghs], B, 3, H),
           "dh0": h0.grad.numpy()}
    return res, _Rec.images


@pytest.mark.parametrize("backend,H,B,T", [("gru16", 32, 2, 5), ("mc", 256, 1, 3)])
def test_references_reproduce_float64_gru(backend, H, B, T):
    nd = 2
    c = gc.case(H, B, T, nd, True, True)
    got = gc.restate32(c, backend)
    free, images = _free64(c, backend)
    # no 16-bit tie flips between the two runs on this shape: the h images both round to are equal, the dgh images
    # equal within 2^-24 (at a gate the planted +-20 saturates, fp32 gives 1 - n^2 = 0 where float64 gives 1e-9)
    hp = gc._hprev(c, got["h"])
    for d in range(nd):
        for s in range(T):
            assert np.array_equal(images["h"][d, s], gc.r16(hp[d, s])), (d, s)
            assert np.abs(images["dgh"][d, s].reshape(B, 3, H) - gc.rbf(got["dgh"][d, s])).max() <= 2.0 ** -24, (d, s)
    er = gc.errors(c, backend, got)
    e_max = max(v[0] for v in er.values())
    ref = dict(gc.ref_fwd64(c, backend, got["h"]), **gc.ref_bwd64(c, backend, got["h"], got["sav"], got["dgh"]))
    tol = {"h": T * er["h"][0] + 1e-12, "r": 1e-12, "z": 1e-12, "n": 1e-12, "ghn": 1e-12}
    for name in gc.OUTS:
        diff = float(np.abs(ref[name] - free[name]).max())
        lim = tol.get(name, 32 * (T + 1) * e_max)
        print(f"{backend} H={H} {name}: |ref64(restate32) - free float64| {diff:.3e} (limit {lim:.3e})")
        assert diff <= lim, (name, diff, lim)


HOST_SHAPE = (6, 6, 1, True, True)
BACKENDS = [("gru16", H) for H in gc.H_GRU16] + [("mc", H) for H in gc.H_MC]


@pytest.mark.parametrize("backend,H", BACKENDS)
def test_gate_passes_restatement_and_rejects_defects(backend, H):
    c = gc.case(H, *HOST_SHAPE)
    er = gc.restate_errors(backend, H, *HOST_SHAPE)
    for name, (e, refmax) in er.items():
        print(f"{backend} H={H} {name}: E_r {e:.3e} max|ref| {refmax:.3g}")
        assert e < 1e-5, (name, e)       # the restatement is an fp32 restatement of the reference
    for defect in gc.DEFECTS:
        ek = gc.errors(c, backend, gc.restate32(c, backend, defect))
        excess = {name: e / gc.gate(e, er[name][0], refmax) for name, (e, refmax) in ek.items()}
        worst = max(excess, key=excess.get)
        print(f"{backend} H={H} {defect}: {excess[worst]:.0f} x the gate in {worst}")
        assert excess[worst] >= 10.0, (defect, excess)
