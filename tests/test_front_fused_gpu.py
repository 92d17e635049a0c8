"""b2p_front_fwd (csrc/front.hip) against the three launches it replaces, bit for bit.

Reference: b2p_gauss_smooth -> b2p_gemm (weights and bias gathered by day, pre_out = z, softsign epilogue, fp32
operands at precision 0 = bf16 MFMA or 2 = fp16 MFMA) -> b2p_cast16_tail, exactly as _FrontEnd.forward and
_ImplicitUnfoldProj.source16 issue them with the fused path switched off. Compared with np.array_equal on the raw
words: xs, z, s and the 16-bit image with its zero tail (bf16 beside precision 0, fp16 beside precision 2, the
pairing the bf16 mode uses). Outputs sit between NaN guard rows.

B = 3 with day indices (2, 0, 2) over 4 days of weights; L = 1 and 19 are shorter than the 20-tap window, 64 is two
32-row blocks exactly, 65 leaves a one-row block, 200 has halos crossing six block edges; 20 taps (even: left 9,
right 10) and 7 taps (odd). A few inputs lie past fp16's range so the saturating conversion of the smoothed
operand is exercised.
"""
import numpy as np
import pytest
import torch

from tests.gru16_cases import Guarded

pytestmark = pytest.mark.gpu

C, DAYS, KTAPS, STRIDE = 256, 4, 32, 4
TAIL = (KTAPS - STRIDE) * C


def _words(t):
    a = t.detach().cpu().contiguous()
    return a.view(torch.int16).numpy().view(np.uint16) if a.element_size() == 2 else a.numpy().view(np.uint32)


def _case(B, L, ntaps, seed, c=C):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, c, generator=g)
    x.view(-1)[:: 211] *= 3.0e5
    taps = torch.rand(ntaps, generator=g) + 0.1
    taps /= taps.sum()
    W = torch.randn(DAYS, c, c, generator=g) / 16.0
    bias = torch.randn(DAYS, 1, c, generator=g)
    day = torch.tensor([2, 0, 2][:B] if B <= 3 else [i % DAYS for i in range(B)], dtype=torch.int64)
    return x.cuda(), taps.cuda(), W.cuda(), bias.cuda(), day.cuda()


def _reference(x, taps, W, bias, day, half):
    from wav2vec2forbrain_amd import _lib
    from wav2vec2forbrain_amd import functional as Fn
    B, L, c = x.shape
    xs, z, s = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    st = _lib.stream_ptr()
    _lib.call("b2p_gauss_smooth", x.data_ptr(), taps.data_ptr(), taps.numel(), xs.data_ptr(), B, L, c, st)
    with Fn.precision("bf16"), Fn.forward_f16(half):
        Fn.gemm(L, c, c, Fn.op(xs, 0, c, True, bs1=L * c), Fn.op(W, 0, c, False, bs1=c * c, gather=day), s, c,
                cbs1=L * c, nz1=B, bias=bias, biasbs1=c, bias_gather=day, pre_out=z, act=Fn.ACT["softsign"])
    n = B * L * c
    s16 = torch.empty(n + TAIL, device="cuda", dtype=torch.float16 if half else torch.bfloat16)
    _lib.call("b2p_cast16_tail", s.data_ptr(), s16.data_ptr(), n, n + TAIL, int(half), st)
    torch.cuda.synchronize()
    return xs, z, s, s16


@pytest.mark.parametrize("half", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("L", [1, 19, 64, 65, 200])
def test_fused_equals_three_launches(L, half):
    from wav2vec2forbrain_amd import _lib
    B = 3
    for ntaps in (20, 7):
        x, taps, W, bias, day = _case(B, L, ntaps, 100 * L + ntaps)
        ref = _reference(x, taps, W, bias, day, half)
        n = B * L * C
        g = Guarded()
        xs, z, s = g.new(n), g.new(n), g.new(n)
        s16f = g.new((n + TAIL) // 2)          # the 16-bit image, (n + TAIL) halfwords, between fp32 guards
        _lib.call("b2p_front_fwd", x.data_ptr(), taps.data_ptr(), ntaps, day.data_ptr(), DAYS, W.data_ptr(),
                  bias.data_ptr(), xs.data_ptr(), z.data_ptr(), s.data_ptr(), s16f.data_ptr(), int(half), TAIL, B, L, C,
                  2 if half else 0, _lib.stream_ptr())
        torch.cuda.synchronize()
        g.check(finite=False)
        s16 = s16f.view(torch.int16)
        for name, r, o in zip(("xs", "z", "s", "s16"), ref, (xs, z, s, s16)):
            rw, ow = _words(r).reshape(-1), _words(o).reshape(-1)
            assert rw.shape == ow.shape, name
            assert np.array_equal(rw, ow), (name, L, ntaps, half, int((rw != ow).sum()))
        assert not _words(s16)[n:].any()        # the zero tail
        assert torch.isfinite(z).all() and torch.isfinite(xs).all()


def test_without_image_and_argument_checks():
    from wav2vec2forbrain_amd import _lib
    lib = _lib.load()
    B, L = 2, 33
    x, taps, W, bias, day = _case(B, L, 20, 5)
    ref = _reference(x, taps, W, bias, day, False)
    g = Guarded()
    n = B * L * C
    xs, z, s = g.new(n), g.new(n), g.new(n)
    args = [x.data_ptr(), taps.data_ptr(), 20, day.data_ptr(), DAYS, W.data_ptr(), bias.data_ptr(), xs.data_ptr(),
            z.data_ptr(), s.data_ptr(), None, 0, 0, B, L, C, 0, _lib.stream_ptr()]
    _lib.call("b2p_front_fwd", *args)
    torch.cuda.synchronize()
    g.check()
    for r, o in zip(ref[:3], (xs, z, s)):
        assert np.array_equal(_words(r).reshape(-1), _words(o).reshape(-1))
    for i, bad in ((15, 64), (2, 65), (16, 1), (12, 2)):   # C, ntaps, precision, tail
        a = list(args)
        a[i] = bad
        assert lib.b2p_front_fwd(*a) != 0


def _spy(monkeypatch):
    from wav2vec2forbrain_amd import _lib
    lib = _lib.load()
    calls = []
    real = lib.b2p_front_fwd

    def spy(*a):
        calls.append(a)
        return real(*a)

    monkeypatch.setattr(lib, "b2p_front_fwd", spy)
    return calls


def _front(x, taps, W, bias, day, fused, half, unfold=(KTAPS, STRIDE)):
    """_FrontEnd forward + backward; (s, image or None, dW, dbias)."""
    from wav2vec2forbrain_amd import functional as Fn
    Wp, bp = W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    old = Fn._FRONT_FUSED[0]
    Fn._FRONT_FUSED[0] = fused
    try:
        with Fn.precision("bf16"):
            with Fn.forward_f16(half):
                s = Fn.front_end(x, day, Wp, bp, taps, unfold=unfold)
                img = Fn._src16_of(s)
            g = torch.Generator().manual_seed(9)
            s.backward(torch.randn(s.shape, generator=g).cuda())
    finally:
        Fn._FRONT_FUSED[0] = old
    torch.cuda.synchronize()
    return s.detach(), img, Wp.grad, bp.grad


@pytest.mark.parametrize("half", [False, True], ids=["bf16", "fp16"])
def test_front_end_gradients_fused_on_and_off(monkeypatch, half):
    calls = _spy(monkeypatch)
    x, taps, W, bias, day = _case(2, 40, 20, 11)
    off = _front(x, taps, W, bias, day, False, half)
    assert calls == [] and off[1] is None
    on = _front(x, taps, W, bias, day, True, half)
    assert len(calls) == 1
    for a, b in zip((off[0], off[2], off[3]), (on[0], on[2], on[3])):
        assert np.array_equal(_words(a), _words(b))
    # the attached image is what the implicit-Unfold projection would have cast: s and (KTAPS - STRIDE) * C zeros
    from wav2vec2forbrain_amd import _lib
    img = on[1]
    n = x.numel()
    assert img is not None and img.numel() == n + TAIL and img.dtype == (torch.float16 if half else torch.bfloat16)
    want = torch.empty_like(img)
    _lib.call("b2p_cast16_tail", on[0].contiguous().data_ptr(), want.data_ptr(), n, n + TAIL, int(half),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_words(want), _words(img))


def test_other_channel_counts_take_the_three_launch_path(monkeypatch):
    calls = _spy(monkeypatch)
    x, taps, W, bias, day = _case(3, 19, 20, 13, c=64)
    off = _front(x, taps, W, bias, day, False, False)
    on = _front(x, taps, W, bias, day, True, False)
    assert calls == [] and on[1] is None
    for a, b in zip((off[0], off[2], off[3]), (on[0], on[2], on[3])):
        assert np.array_equal(_words(a), _words(b))
