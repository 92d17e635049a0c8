"""Multi-CU persistent GRU recurrence at hidden size 1024 (csrc/grumc.hip: b2p_gru_fwd_mc / b2p_gru_bwd_mc) on
the device.

The direct cases hold every output (out, saved, dgi, dgh, dh0) against a float64 evaluation of the same
recurrence on the CPU, with a bound MEASURED in the same test from the unchanged H = 512 instantiation of the
same kernels against its own float64 reference, at the same (B, T, ndir, h0, bias) and seed rule:

    E_1024 <= 2 * E_512 + 1e-6        (relative L2 errors against float64, per output)

Both sizes round the same things (W_hh and h to fp16 in the forward, W_hh and dgh to bf16 in the backward) and
accumulate in fp32; an emulation of those roundings gives H = 1024 / H = 512 error ratios of 0.99 - 1.01 (out,
dgi; absolute 1.1 - 1.4e-4 and 5.7 - 7.8e-4), so a factor 2 is slack while a wrong unit, gate or batch index
misses by orders of magnitude. The float64 side restates the gate equations forward and gets dgi / dh0 from
autograd; dgh is (dgi_r, dgi_z, dgi_n * r) by the chain rule. The layer-level cases apply the same bound to
Fn.gru_layer's output and gradients, calibrated against the same layer at H = 512."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, T, ndir, h0, bias) at H = 1024 (and, for the bound, at H = 512)
DIRECT = [(5, 1, 2, True, True),       # single step: no exchange, partial group
          (17, 2, 2, False, True),     # two groups, both exchange parities, NULL h0 / dh0
          (17, 3, 1, True, False),     # first slot reuse, NULL bhh, one direction
          (33, 41, 2, True, True),     # error accumulates
          (65, 3, 2, False, True)]     # 2 * 5 * 16 = 160 workgroups > the 128 of one launch: chunked
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


def _run(ins, H, B, T, nd):
    """b2p_gru_fwd_mc + b2p_gru_bwd_mc -> (out, saved, dgi, dgh, dh0 or None, the fail word after each pass)."""
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
    ws = torch.empty(int(_lib.load().b2p_gru_mc_workspace(B, H, nd)), device=dev, dtype=torch.uint8)
    _lib.call("b2p_gru_fwd_mc", p(gi), p(whh), p(bhh), p(h0), p(out), p(sv), p(ws), B, T, H, nd, st)
    f1 = ws[:4].clone()
    _lib.call("b2p_gru_bwd_mc", p(dout), p(whh), p(out), p(sv), p(h0), p(dgi), p(dgh), p(dh0), p(ws), B, T, H, nd, st)
    return out, sv, dgi, dgh, dh0, torch.cat([f1, ws[:4]])


def _dev(ins):
    return tuple(None if t is None else t.cuda() for t in ins)


def _errors(H, B, T, nd, has_h0, has_bias):
    ins, ref = _case(H, B, T, nd, has_h0, has_bias)
    res = _run(_dev(ins), H, B, T, nd)
    torch.cuda.synchronize()
    assert int(res[5].abs().sum()) == 0, f"H={H}: a member timed out"
    return [None if r is None else _rel64(a, r) for a, r in zip(res[:5], ref)], res


@pytest.mark.parametrize("B,T,nd,has_h0,has_bias", DIRECT)
def test_direct_against_float64(B, T, nd, has_h0, has_bias):
    """1. Every output at H = 1024 is as close to float64 as the H = 512 kernels' at the same shape (factor 2
    + 1e-6, relative L2), and no member timed out (the fail word after the forward and after the backward)."""
    e512, _ = _errors(512, B, T, nd, has_h0, has_bias)
    e1024, res = _errors(1024, B, T, nd, has_h0, has_bias)
    assert (res[4] is None) == (not has_h0)
    for name, e_new, e_old in zip(NAMES, e1024, e512):
        if e_new is None:
            assert name == "dh0" and not has_h0 and e_old is None
            continue
        print(f"grumc direct B={B} T={T} nd={nd} {name}: H=1024 {e_new:.3e} H=512 {e_old:.3e}")
    for name, e_new, e_old in zip(NAMES, e1024, e512):
        if e_new is not None:
            assert e_new <= 2 * e_old + 1e-6, (name, e_new, e_old)


@pytest.mark.parametrize("H,B,T", [(1024, 33, 7), (1024, 65, 3), (512, 33, 7)])
def test_deterministic_and_graph_replay(H, B, T):
    """2. / 4. Two eager runs are bitwise equal, and a captured graph of forward + backward replayed three times
    reproduces them bit for bit with the fail word 0 every time (the workspace is zeroed by a node of the
    graph, so the tags of the previous replay never match). H = 512: the same, as before."""
    ins, _ = _case(H, B, T, 2, True, True)
    di = _dev(ins)
    a = _run(di, H, B, T, 2)
    b = _run(di, H, B, T, 2)
    torch.cuda.synchronize()
    assert int(a[5].abs().sum()) == 0 and int(b[5].abs().sum()) == 0
    for x, y in zip(a[:5], b[:5]):
        assert torch.equal(x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(di, H, B, T, 2)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        res = _run(di, H, B, T, 2)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert int(res[5].abs().sum()) == 0
        for x, y in zip(res[:5], a[:5]):
            assert torch.equal(x, y)


@functools.lru_cache(maxsize=None)
def _layer_case(H, unfold):
    """Fn.gru_layer's inputs (fp32, CPU) at IN = 64, B = 4, T = 12, two directions, with an initial state, and
    the float64 output and gradients (x, then W_ih, W_hh, b_ih, b_hh per direction, then h0)."""
    from oracle.b2p2t_oracle import gru_direction, unfold as unfold_ref
    g = torch.Generator().manual_seed(9000 + H + int(unfold))
    B, T, IN, k, s = 4, 12, 64, 8, 4
    xsrc = torch.randn(B, (T - 1) * s + k, IN // k, generator=g) if unfold else torch.randn(B, T, IN, generator=g)
    ws = []
    for d in range(2):
        ws += [torch.randn(3 * H, IN, generator=g) / math.sqrt(IN), torch.randn(3 * H, H, generator=g) / math.sqrt(H),
               torch.randn(3 * H, generator=g) * 0.1, torch.randn(3 * H, generator=g) * 0.1]
    hz = torch.randn(2, B, H, generator=g)
    wr = [w.double().requires_grad_(True) for w in ws]
    xr = xsrc.double().requires_grad_(True)
    hr = hz.double().requires_grad_(True)
    xin = unfold_ref(xr, k, s) if unfold else xr
    ref = torch.cat([gru_direction(xin, *wr[4 * d:4 * d + 4], hr[d], d == 1) for d in range(2)], -1)
    assert ref.shape == (B, T, 2 * H)
    dout = torch.randn(B, T, 2 * H, generator=g)
    refg = torch.autograd.grad(ref, [xr, *wr, hr], dout.double())
    return xsrc, ws, hz, dout, [ref.detach(), *refg], (k, s)


def _layer_errors(H, unfold):
    Fn = _fn()
    xsrc, ws, hz, dout, ref, ks = _layer_case(H, unfold)
    with Fn.precision("bf16"):
        wg = [w.cuda().requires_grad_(True) for w in ws]
        xs = xsrc.cuda().requires_grad_(True)
        hg = hz.cuda().requires_grad_(True)
        out = Fn.gru_layer(Fn.Unfolded(xs, *ks) if unfold else xs, H, 2, wg, hg)
        assert out.grad_fn.meta[-3:] == (False, True, False), f"H={H}: not the multi-CU recurrence"   # (16, mc, 32)
        got = torch.autograd.grad(out, [xs, *wg, hg], dout.cuda())
    torch.cuda.synchronize()
    return [_rel64(a, r) for a, r in zip([out.detach(), *got], ref)]


@pytest.mark.parametrize("unfold", [False, True])
def test_gru_layer_bf16(unfold):
    """3. Fn.gru_layer under precision('bf16') at H = 1024 takes "mc" (ctx.meta); its output and every gradient
    are within the factor-2 bound of the same layer at H = 512, and the status word stays 0."""
    Fn = _fn()
    e512 = _layer_errors(512, unfold)
    e1024 = _layer_errors(1024, unfold)
    names = ["out", "dx"] + [f"d{n}{d}" for d in range(2) for n in ("W_ih", "W_hh", "b_ih", "b_hh")] + ["dh0"]
    for name, e_new, e_old in zip(names, e1024, e512):
        print(f"grumc layer unfold={unfold} {name}: H=1024 {e_new:.3e} H=512 {e_old:.3e}")
    for name, e_new, e_old in zip(names, e1024, e512):
        assert e_new <= 2 * e_old + 1e-6, (name, e_new, e_old)
    assert Fn.gru_status_value() == 0


def test_tiny_model_step():
    """5. Trainer.train_step on the smallest trainer-test configuration with a GRU of hidden size 1024: the eager
    first step and the replayed steps give finite losses that agree with a Trainer that never replays
    (tests/test_trainer_gpu.py's tolerance), and the status word stays 0."""
    from tests.helpers import CFG, build_model, batch_dict
    from wav2vec2forbrain_amd.datasets.batch_types import make_b2t_batch
    from wav2vec2forbrain_amd.train.train_loop import Trainer
    from wav2vec2forbrain_amd.workloads import SyntheticStepExperiment
    Fn = _fn()
    cfg = dict(CFG["plumbing_base"], gru_hidden=1024)
    b = batch_dict(cfg)
    batch = make_b2t_batch(b["x"], b["target"], b["day_idxs"], b["input_lens"], b["target_lens"]).cuda()
    res = []
    for graphs in (False, True):
        model = build_model(cfg)
        model.train()
        with Fn.precision("bf16"):
            assert Fn._gru_recurrence(1024) == "mc"
            trainer = Trainer(SyntheticStepExperiment(model, lr=1e-3, gradient_clipping=None))
            trainer.use_graphs = graphs
            trainer.capture_after = 1
            losses = [float(trainer.train_step(batch).metrics["ctc_loss"]) for _ in range(3)]
        torch.cuda.synchronize()
        if graphs:
            assert (trainer.eager_steps, trainer.graph_steps) == (1, 2)
        res.append(losses)
        trainer.release_graphs()
        Fn.set_deferred_wgrad([])
    print(f"grumc H=1024 train_step losses: eager {res[0]} replayed {res[1]}")
    assert all(math.isfinite(v) for v in res[0] + res[1])
    np.testing.assert_allclose(res[1], res[0], rtol=1e-5, atol=0)
    assert Fn.gru_status_value() == 0


def test_status_word_clean():
    """After everything above no launch has folded a timeout into the persistent status word."""
    assert _fn().gru_status_value() == 0
