"""csrc/skinny32.hip against gemm_kernel (csrc/gemm.hip), bit for bit.

The three skinny forms of a 32-wide head (forward C[M][32] = A W^T + bias, input gradient dA[M][K] = dC W, weight
gradient dW[32][K] = dC^T A) run the descriptor b2p_gemm would run, and every output word must equal b2p_gemm's
(np.array_equal on the uint32 views) at both precisions that have a form: 0 (bf16 MFMA, the backward of the bf16
mode) and 2 (fp16 MFMA, its forward under forward_f16). M covers one row, a partial / full / just-over 16-row MFMA
tile, a row block plus one row, and several workgroups; K covers a single float4, one 64-wide K tile and the head's
768. Outputs sit between NaN guard rows. The weight gradient at M = 7968 goes through functional.mm_tn with the
dispatch switch on and off: functional.gemm picks ksplit = 7, kchunk = 1152 there, and both paths sum those slabs
with the same reduce kernel.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.gru16_cases import Guarded

pytestmark = pytest.mark.gpu

MS = (1, 15, 16, 17, 33, 250)
KS = (4, 64, 768)
FWD, DGRAD, WGRAD = 1, 2, 3


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _inputs(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    x.view(-1)[:: 97] *= 1.0e5   # past fp16's range: precision 2 saturates these while staging
    return x.cuda()


def _desc(form, M, K, prec, a, b, out, bias=None, ksplit=0, kchunk=0, ws=None):
    """The descriptor functional.gemm builds for mm_nt / mm_nn / mm_tn of a Linear(K -> 32) over M rows."""
    from wav2vec2forbrain_amd import _lib
    from wav2vec2forbrain_amd import functional as Fn
    d = _lib.GemmDesc()
    if form == FWD:      # a (M, K), b = W (32, K)
        d.M, d.N, d.K = M, 32, K
        d.A, d.B, ldc = Fn.op(a, 0, K, True), Fn.op(b, 0, K, True), 32
    elif form == DGRAD:  # a = dC (M, 32), b = W (32, K)
        d.M, d.N, d.K = M, K, 32
        d.A, d.B, ldc = Fn.op(a, 0, 32, True), Fn.op(b, 0, K, False), K
    else:                # a = dC (M, 32), b = x (M, K)
        d.M, d.N, d.K = 32, K, M
        d.A, d.B, ldc = Fn.op(a, 0, 32, False), Fn.op(b, 0, K, False), K
    d.nz1 = d.nz2 = 1
    e = _lib.Epilogue()
    e.C, e.ldc, e.alpha, e.beta = out.data_ptr(), ldc, 1.0, 0.0
    e.bias = None if bias is None else bias.data_ptr()
    e.ldaux = e.ldr = ldc
    d.ep = e
    d.precision = prec
    if ksplit > 1:
        d.ksplit, d.kchunk, d.workspace, d.workspace_floats = ksplit, kchunk, ws.data_ptr(), ws.numel()
    return d


def _run_both(form, M, K, prec, bias, seed, ksplit=0, kchunk=0):
    from wav2vec2forbrain_amd import _lib
    lib = _lib.load()
    st = _lib.stream_ptr()
    if form == FWD:
        a, b, n_out = _inputs(M, K, seed), _inputs(32, K, seed + 1), M * 32
    elif form == DGRAD:
        a, b, n_out = _inputs(M, 32, seed), _inputs(32, K, seed + 1), M * K
    else:
        a, b, n_out = _inputs(M, 32, seed), _inputs(M, K, seed + 1), 32 * K
    bv = _inputs(1, 32, seed + 2).view(-1) if bias else None
    g = Guarded()
    outs = []
    for fn in (lib.b2p_gemm, lib.b2p_skinny32):
        out = g.new(n_out)
        ws = g.new(ksplit * n_out) if ksplit > 1 else None
        d = _desc(form, M, K, prec, a, b, out, bv, ksplit, kchunk, ws)
        assert lib.b2p_skinny32_form(ctypes.byref(d)) == form
        _lib.check(fn(ctypes.byref(d), st), fn.__name__)
        outs.append(out)
    torch.cuda.synchronize()
    g.check(finite=False)
    ref, got = _bits(outs[0]), _bits(outs[1])
    assert not np.isnan(outs[0].cpu().numpy()).any(), (form, M, K, prec)
    assert np.array_equal(ref, got), (form, M, K, prec, bias, int((ref != got).sum()))


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("form", [FWD, DGRAD, WGRAD])
def test_bitwise_against_gemm_kernel(form, prec):
    seed = 1000 * form + 10 * prec
    for M in MS:
        for K in KS:
            for bias in ((False, True) if form == FWD else (False,)):
                seed += 3
                _run_both(form, M, K, prec, bias, seed)


@pytest.mark.parametrize("prec", [0, 2])
def test_wgrad_explicit_split(prec):
    """Split-K through the C ABI: 250 rows in 4 slices of 64 (the last one partial), then the reduce."""
    _run_both(WGRAD, 250, 768, prec, False, 77, ksplit=4, kchunk=64)
    _run_both(WGRAD, 250, 4, prec, False, 78, ksplit=2, kchunk=128)


def _spy(monkeypatch):
    from wav2vec2forbrain_amd import _lib
    lib = _lib.load()
    calls = []
    real = lib.b2p_skinny32

    def spy(d, st):
        o = d._obj
        calls.append((int(o.M), int(o.N), int(o.K), int(o.ksplit), int(o.kchunk)))
        return real(d, st)

    monkeypatch.setattr(lib, "b2p_skinny32", spy)
    return calls


@pytest.mark.parametrize("M", [250, 7968])
def test_functional_dispatch_head(monkeypatch, M):
    """functional.mm_nt / mm_nn / mm_tn of a Linear(768 -> 32): switch on (skinny32) against switch off."""
    from wav2vec2forbrain_amd import functional as Fn
    calls = _spy(monkeypatch)
    x, W, bias, dy = _inputs(M, 768, 5), _inputs(32, 768, 6), _inputs(1, 32, 7).view(-1), _inputs(M, 32, 8)
    res = {}
    for on in (False, True):
        old = Fn._SKINNY32[0]
        Fn._SKINNY32[0] = on
        try:
            with Fn.precision("bf16"):
                y, dx, dw = torch.empty(M, 32, device="cuda"), torch.empty(M, 768, device="cuda"), \
                    torch.empty(32, 768, device="cuda")
                with Fn.forward_f16():
                    Fn.mm_nt(x, W, y, bias=bias)
                Fn.mm_nn(dy, W, dx)
                Fn.mm_tn(dy, x, dw)
        finally:
            Fn._SKINNY32[0] = old
        torch.cuda.synchronize()
        res[on] = (y, dx, dw)
        if not on:
            assert calls == []
    assert [c[:3] for c in calls] == [(M, 32, 768), (M, 768, 32), (32, 768, M)]
    if M == 7968:   # the K partition functional.gemm picks for the head's weight gradient
        assert calls[2][3:] == (7, 1152)
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(_bits(a), _bits(b))


def test_other_widths_fall_back(monkeypatch):
    """N = 40, the fp32 parity mode and an epilogue beyond a bias stay on gemm_kernel."""
    from wav2vec2forbrain_amd import _lib
    from wav2vec2forbrain_amd import functional as Fn
    calls = _spy(monkeypatch)
    x, W40, W32 = _inputs(33, 64, 1), _inputs(40, 64, 2), _inputs(32, 64, 3)
    y40, y32 = torch.empty(33, 40, device="cuda"), torch.empty(33, 32, device="cuda")
    with Fn.precision("bf16"):
        Fn.mm_nt(x, W40, y40)
        Fn.mm_nt(x, W32, y32, act=Fn.ACT["gelu"])
        Fn.mm_nt(x, W32, y32, alpha=0.5)
    with Fn.precision("fp32"):
        Fn.mm_nt(x, W32, y32)
    torch.cuda.synchronize()
    assert calls == []
    d = _desc(FWD, 33, 64, 0, x, W32, y32)
    d.N = 40
    lib = _lib.load()
    assert lib.b2p_skinny32_form(ctypes.byref(d)) == 0
    assert lib.b2p_skinny32(ctypes.byref(d), _lib.stream_ptr()) != 0
    assert b"b2p_gemm" in lib.b2p_last_error()
