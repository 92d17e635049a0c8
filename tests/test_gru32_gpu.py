"""Persistent exact-fp32 GRU recurrence (csrc/gru32.hip: b2p_gru_fwd32 / b2p_gru_bwd32) on the device.

The direct cases hold every output (out, saved, dgi, dgh, dh0) against a float64 evaluation of the same
recurrence on the CPU, with a bound MEASURED in the same test from the unchanged per-step kernels
(b2p_gru_fwd / b2p_gru_bwd):

    E_new <= 2 * E_step + 1e-7        (relative L2 errors against float64, per output)

Both forms are fp32 sums of the same lengths in another order (fmaf chains of H/4 terms per gate against a
4-way split of K); a factor 2 absorbs that, while a 16-bit rounding anywhere would miss by orders of
magnitude. The float64 side restates the gate equations forward and gets dgi / dh0 from autograd; dgh is
(dgi_r, dgi_z, dgi_n * r) by the chain rule."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (H, B, T, ndir, h0, bias)
DIRECT = [(256, 5, 1, 2, True, True),      # single step: no exchange, partial group
          (256, 17, 2, 2, False, True),    # two groups, both exchange parities
          (512, 33, 7, 2, True, False),    # three groups, odd T, NULL bhh
          (512, 8, 57, 1, True, True),     # one direction, the Conformer fine-tune's batch, error accumulates
          (512, 65, 3, 2, False, True)]    # 2 * 5 * 16 = 160 workgroups > the 128 of one launch: chunked
NAMES = ("out", "saved", "dgi", "dgh", "dh0")


def _fn():
    from wav2vec2forbrain_amd import functional as Fn
    return Fn


def _rel64(a, ref):
    return float((a.double().cpu() - ref).norm() / ref.norm())


@functools.lru_cache(maxsize=None)
def _case(H, B, T, nd, has_h0, has_bias):
    """CPU inputs (fp32) and the float64 reference outputs of one shape; computed once, never modified."""
    g = torch.Generator().manual_seed(7000 + H + 31 * B + T)
    gi = torch.randn(B, T, nd * 3 * H, generator=g)
    whh = torch.randn(nd, 3 * H, H, generator=g) / math.sqrt(H)
    bhh = torch.randn(nd, 3 * H, generator=g) * 0.1 if has_bias else None
    h0 = torch.randn(nd, B, H, generator=g) if has_h0 else None
    dout = torch.randn(B, T, nd * H, generator=g)
    gi64 = gi.double().requires_grad_(True)
    h064 = h0.double().requires_grad_(True) if has_h0 else None
    outs, saved = [], torch.zeros(B, T, nd, 4, H, dtype=torch.float64)
    for d in range(nd):
        W = whh[d].double()
        bb = bhh[d].double() if has_bias else torch.zeros(3 * H, dtype=torch.float64)
        h = h064[d] if has_h0 else torch.zeros(B, H, dtype=torch.float64)
        hs = [None] * T
        for t in (range(T - 1, -1, -1) if d == 1 else range(T)):
            gh = h @ W.t() + bb
            gir = gi64[:, t, d * 3 * H:(d + 1) * 3 * H]
            r = torch.sigmoid(gir[:, :H] + gh[:, :H])
            z = torch.sigmoid(gir[:, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gir[:, 2 * H:] + r * gh[:, 2 * H:])
            h = (1 - z) * n + z * h
            hs[t] = h
            saved[:, t, d] = torch.stack([r, z, n, gh[:, 2 * H:]], 1).detach()
        outs.append(torch.stack(hs, 1))
    out = torch.cat(outs, -1)
    grads = torch.autograd.grad(out, [gi64] + ([h064] if has_h0 else []), dout.double())
    dgi = grads[0]
    dgh = dgi.clone().view(B, T, nd, 3, H)
    dgh[:, :, :, 2] *= saved[:, :, :, 0]
    ref = (out.detach(), saved, dgi, dgh.view(B, T, nd * 3 * H), grads[1] if has_h0 else None)
    return (gi, whh, bhh, h0, dout), ref


def _run(form, ins, H, B, T, nd):
    """form 'new' / 'step' -> (out, saved, dgi, dgh, dh0 or None, fail words or None) on the device."""
    from wav2vec2forbrain_amd import _lib
    gi, whh, bhh, h0, dout = ins
    dev = gi.device
    p = lambda t: None if t is None else t.data_ptr()
    out = torch.empty(B, T, nd * H, device=dev)
    sv = torch.empty(B, T, nd, 4, H, device=dev)
    dgi = torch.empty(B, T, nd * 3 * H, device=dev)
    dgh = torch.empty_like(dgi)
    dh0 = torch.empty(nd, B, H, device=dev) if h0 is not None else None
    st = _lib.stream_ptr()
    if form == "new":
        ws = torch.empty(int(_lib.load().b2p_gru32_workspace(B, H, nd)), device=dev, dtype=torch.uint8)
        _lib.call("b2p_gru_fwd32", p(gi), p(whh), p(bhh), p(h0), p(out), p(sv), p(ws), B, T, H, nd, st)
        f1 = ws[:4].clone()
        _lib.call("b2p_gru_bwd32", p(dout), p(whh), p(out), p(sv), p(h0), p(dgi), p(dgh), p(dh0), p(ws), B, T, H, nd, st)
        return out, sv, dgi, dgh, dh0, torch.cat([f1, ws[:4]])
    buf = torch.empty(nd, B, H, device=dev)
    _lib.call("b2p_gru_fwd", p(gi), p(whh), p(bhh), p(h0), p(out), p(sv), B, T, H, nd, st)
    _lib.call("b2p_gru_bwd", p(dout), p(whh), p(out), p(sv), p(h0), p(dgi), p(dgh), p(dh0), p(buf), B, T, H, nd, st)
    return out, sv, dgi, dgh, dh0, None


def _dev(ins):
    return tuple(None if t is None else t.cuda() for t in ins)


@pytest.mark.parametrize("H,B,T,nd,has_h0,has_bias", DIRECT)
def test_direct_against_float64(H, B, T, nd, has_h0, has_bias):
    """1. Every output of the new entry points is as close to float64 as the per-step kernels' (factor 2 +
    1e-7, relative L2), and no member timed out (the fail word after the forward and after the backward)."""
    ins, ref = _case(H, B, T, nd, has_h0, has_bias)
    di = _dev(ins)
    step = _run("step", di, H, B, T, nd)
    new = _run("new", di, H, B, T, nd)
    torch.cuda.synchronize()
    assert int(new[5].abs().sum()) == 0, "a member timed out"
    for name, a, s, r in zip(NAMES, new[:5], step[:5], ref):
        if r is None:
            assert a is None
            continue
        e_new, e_step = _rel64(a, r), _rel64(s, r)
        print(f"gru32 direct H={H} B={B} T={T} nd={nd} {name}: new {e_new:.3e} per-step {e_step:.3e}")
        assert e_new <= 2 * e_step + 1e-7, (name, e_new, e_step)


@pytest.mark.parametrize("H,B,T", [(512, 33, 7), (256, 17, 2)])
def test_deterministic_and_graph_replay(H, B, T):
    """2. Two eager runs are bitwise equal, and a captured graph of forward + backward replayed three times
    reproduces them bit for bit with the fail word 0 every time (the workspace is zeroed by a node of the
    graph, so the tags of the previous replay never match)."""
    ins, _ = _case(H, B, T, 2, True, H == 256)
    di = _dev(ins)
    a = _run("new", di, H, B, T, 2)
    b = _run("new", di, H, B, T, 2)
    torch.cuda.synchronize()
    assert int(a[5].abs().sum()) == 0 and int(b[5].abs().sum()) == 0
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run("new", di, H, B, T, 2)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        res = _run("new", di, H, B, T, 2)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(res[5].abs().sum()) == 0
        for x, y in zip(res[:5], a[:5]):
            assert torch.equal(x, y)


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _layer_case(H, B, unfold, h0):
    from oracle.b2p2t_oracle import gru_direction, unfold as unfold_ref
    torch.manual_seed(3)
    k, s = 8, 4
    if unfold:
        xsrc = torch.randn(B, 96, 16)     # T = (96 - 8) / 4 + 1 = 23
    else:
        xsrc = torch.randn(B, 23, 48)
    IN = 16 * k if unfold else 48
    ws = []
    for d in range(2):
        ws += [torch.randn(3 * H, IN) / math.sqrt(IN), torch.randn(3 * H, H) / math.sqrt(H), torch.randn(3 * H) * 0.1,
               torch.randn(3 * H) * 0.1]
    hz = torch.randn(2, B, H) if h0 else None
    wr = [w.clone().requires_grad_(True) for w in ws]
    xr = xsrc.clone().requires_grad_(True)
    xin_ref = unfold_ref(xr, k, s) if unfold else xr
    hr = hz.clone().requires_grad_(True) if h0 else None
    ref = torch.cat([gru_direction(xin_ref, *wr[4 * d:4 * d + 4], hr[d] if h0 else None, d == 1) for d in range(2)], -1)
    dout = torch.randn_like(ref)
    refg = torch.autograd.grad(ref, [xr, *wr] + ([hr] if h0 else []), dout)
    return xsrc, ws, hz, ref.detach(), dout, refg, (k, s)


def _layer(Fn, xsrc, ws, hz, unfold, ks, H):
    wg = [w.cuda().requires_grad_(True) for w in ws]
    xs = xsrc.cuda().requires_grad_(True)
    x_in = Fn.Unfolded(xs, *ks) if unfold else xs
    hg = hz.cuda().requires_grad_(True) if hz is not None else None
    out = Fn.gru_layer(x_in, H, 2, wg, hg)
    return out, [xs, *wg] + ([hg] if hz is not None else [])


@pytest.mark.parametrize("unfold", [False, True])
@pytest.mark.parametrize("h0", [False, True])
@pytest.mark.parametrize("H", [256, 512])
def test_gru_layer_bf16x3(unfold, h0, H):
    """3. Fn.gru_layer under the bf16x3 mode (B 13, T 23) against the oracle GRU with test_gru_layer's
    tolerances (output < 1e-4, every gradient < 2e-4); the layer took the persistent exact-fp32 kernels
    (ctx.meta), and under persistent_gru32(False) it takes the per-step kernels."""
    Fn = _fn()
    B = 13
    xsrc, ws, hz, ref, dout, refg, ks = _layer_case(H, B, unfold, h0)
    with Fn.precision("bf16x3"):
        out, leaves = _layer(Fn, xsrc, ws, hz, unfold, ks, H)
        assert out.grad_fn.meta[-3:] == (False, False, True)      # (use16, usemc, use32)
        assert _rel(out.detach().cpu(), ref) < 1e-4
        got = torch.autograd.grad(out, leaves, dout.cuda())
        with Fn.persistent_gru32(False):
            out_s, _ = _layer(Fn, xsrc, ws, hz, unfold, ks, H)
            assert out_s.grad_fn.meta[-3:] == (False, False, False)
        assert _rel(out_s.detach().cpu(), ref) < 1e-4
    for i, (a, b) in enumerate(zip(got, refg)):
        assert _rel(a.cpu(), b) < 2e-4, (i, _rel(a.cpu(), b))
    Fn.check_gru_status()


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_other_modes_untouched(mode):
    """4. Outside GRU32_MODES the switch selects nothing: the layer's outputs and gradients with
    persistent_gru32 on and off are bitwise equal, and the new kernels are not taken."""
    Fn = _fn()
    assert Fn.PRECISION_MODES[mode] not in Fn.GRU32_MODES and Fn.PRECISION_MODES["bf16x3"] in Fn.GRU32_MODES
    H, B = 512, 13
    xsrc, ws, hz, ref, dout, refg, ks = _layer_case(H, B, False, True)
    res = []
    for on in (True, False):
        with Fn.precision(mode), Fn.persistent_gru32(on):
            out, leaves = _layer(Fn, xsrc, ws, hz, False, ks, H)
            assert out.grad_fn.meta[-1] is False
            res.append([out.detach()] + list(torch.autograd.grad(out, leaves, dout.cuda())))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_status_word_clean():
    """5. After everything above no launch has folded a timeout into the persistent status word."""
    assert _fn().gru_status_value() == 0
