"""Persistent exact-fp32 GRU recurrence at hidden size 1024 (csrc/gru32.hip: gru32_fwd<1024> / gru32_bwd<1024>,
P = 32 members per recurrence) on the device.

The direct cases hold every output against a float64 evaluation of the same recurrence on the CPU (the _case of
tests/test_gru32_gpu.py), with bounds MEASURED in the same test (relative L2 errors against float64, per output):

    forward  (out, saved)    : E_1024 <= 2 * E_step + 1e-7   the unchanged per-step forward at H = 1024
    backward (dgi, dgh, dh0) : E_1024 <= 2 * E_512  + 1e-7   gru32<512> at the same shape (no other backward
                                                             exists at this size)

A chain twice as long can at worst double the error (a plain fp32 restatement on the CPU gives 1024 / 512 ratios
of 1.04 to 1.16 at these shapes and seeds, on out, dgi and dh0); a 16-bit rounding anywhere would miss either
bound by orders of magnitude."""
import math

import numpy as np
import pytest
import torch

from tests.test_gru32_gpu import NAMES, _case, _dev, _rel64, _run

pytestmark = pytest.mark.gpu

H = 1024
# (B, T, ndir, h0, bias)
DIRECT = [(5, 1, 2, True, True),       # no exchange, a partial group
          (17, 2, 2, False, True),     # two groups, both parities, NULL h0 / dh0
          (17, 3, 1, True, False),     # the first slot reuse, NULL bhh, one direction
          (33, 7, 2, True, True),      # three batch groups, so two launches
          (8, 41, 1, True, True),      # the fine-tune's batch, error accumulates
          (65, 3, 2, False, True)]     # three launches


def _fn():
    from wav2vec2forbrain_amd import functional as Fn
    return Fn


def _step_fwd(ins, B, T, nd):
    """The per-step forward (b2p_gru_fwd; it has no backward at this size) -> (out, saved)."""
    from wav2vec2forbrain_amd import _lib
    gi, whh, bhh, h0, _ = ins
    p = lambda t: None if t is None else t.data_ptr()
    out = torch.empty(B, T, nd * H, device=gi.device)
    sv = torch.empty(B, T, nd, 4, H, device=gi.device)
    _lib.call("b2p_gru_fwd", p(gi), p(whh), p(bhh), p(h0), p(out), p(sv), B, T, H, nd, _lib.stream_ptr())
    return out, sv


def _errors512(B, T, nd, has_h0, has_bias):
    """gru32<512>'s errors against float64 at the same shape: the backward's yardstick."""
    ins, ref = _case(512, B, T, nd, has_h0, has_bias)
    res = _run("new", _dev(ins), 512, B, T, nd)
    torch.cuda.synchronize()
    assert int(res[5].abs().sum()) == 0, "H=512: a member timed out"
    return [None if r is None else _rel64(a, r) for a, r in zip(res[:5], ref)]


@pytest.mark.parametrize("B,T,nd,has_h0,has_bias", DIRECT)
def test_direct_against_float64(B, T, nd, has_h0, has_bias):
    """1. Forward outputs within the bound of the per-step forward at H = 1024, backward outputs within the bound
    of gru32<512> at the same shape, and no member timed out (the fail word after either pass)."""
    ins, ref = _case(H, B, T, nd, has_h0, has_bias)
    di = _dev(ins)
    step = _step_fwd(di, B, T, nd)
    new = _run("new", di, H, B, T, nd)
    torch.cuda.synchronize()
    e512 = _errors512(B, T, nd, has_h0, has_bias)
    assert (new[4] is None) == (not has_h0)
    e_new = [None if r is None else _rel64(a, r) for a, r in zip(new[:5], ref)]
    e_old = [_rel64(step[0], ref[0]), _rel64(step[1], ref[1])] + e512[2:]
    for name, a, b in zip(NAMES, e_new, e_old):
        if a is not None:
            print(f"gru32 H=1024 B={B} T={T} nd={nd} {name}: {a:.3e} against "
                  f"{'per-step H=1024' if name in ('out', 'saved') else 'gru32 H=512'} {b:.3e}")
    assert int(new[5].abs().sum()) == 0, "a member timed out"
    for name, a, b in zip(NAMES, e_new, e_old):
        if a is not None:
            assert a <= 2 * b + 1e-7, (name, a, b)


def test_backward_consumes_the_per_step_forward():
    """2. b2p_gru_bwd32 fed the per-step forward's out / saved (the layouts are shared) meets the same bound."""
    from wav2vec2forbrain_amd import _lib
    B, T, nd = 17, 3, 1
    ins, ref = _case(H, B, T, nd, True, False)
    gi, whh, bhh, h0, dout = di = _dev(ins)
    out, sv = _step_fwd(di, B, T, nd)
    dgi = torch.empty(B, T, nd * 3 * H, device="cuda")
    dgh = torch.empty_like(dgi)
    dh0 = torch.empty(nd, B, H, device="cuda")
    ws = torch.empty(int(_lib.load().b2p_gru32_workspace(B, H, nd)), device="cuda", dtype=torch.uint8)
    _lib.call("b2p_gru_bwd32", dout.data_ptr(), whh.data_ptr(), out.data_ptr(), sv.data_ptr(), h0.data_ptr(),
              dgi.data_ptr(), dgh.data_ptr(), dh0.data_ptr(), ws.data_ptr(), B, T, H, nd, _lib.stream_ptr())
    torch.cuda.synchronize()
    e512 = _errors512(B, T, nd, True, False)
    errs = [_rel64(a, r) for a, r in zip((dgi, dgh, dh0), ref[2:])]
    for name, a, b in zip(NAMES[2:], errs, e512[2:]):
        print(f"gru32 H=1024 backward of the per-step forward {name}: {a:.3e} against gru32 H=512 {b:.3e}")
    assert int(ws[:4].view(torch.int32).item()) == 0, "a member timed out"
    for name, a, b in zip(NAMES[2:], errs, e512[2:]):
        assert a <= 2 * b + 1e-7, (name, a, b)


def test_deterministic_and_graph_replay():
    """3. Two eager runs are bitwise equal, and a captured forward + backward replayed three times reproduces them
    bit for bit with the fail word 0 every time (two launches per pass, the workspace zeroed by a graph node)."""
    B, T = 33, 7
    ins, _ = _case(H, B, T, 2, True, True)
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


@pytest.mark.parametrize("unfold", [False, True])
def test_gru_layer_bf16x3(unfold):
    """4. Fn.gru_layer under precision('bf16x3') with the 'gru32w' form (B 4, T 12, IN 64: the layer case of
    tests/test_gru_mc1024_gpu.py) takes the persistent exact-fp32 kernels (ctx.meta) and meets
    test_gru_layer_bf16x3's tolerances against the oracle: output < 1e-4, every gradient < 2e-4."""
    from tests.test_gru_mc1024_gpu import _layer_case
    Fn = _fn()
    xsrc, ws, hz, dout, ref, ks = _layer_case(H, unfold)
    with Fn.precision("bf16x3"), Fn.x3_forms({"gru32w"}):     # the form alone: every GEMM stays three-term
        wg = [w.cuda().requires_grad_(True) for w in ws]
        xs = xsrc.cuda().requires_grad_(True)
        hg = hz.cuda().requires_grad_(True)
        out = Fn.gru_layer(Fn.Unfolded(xs, *ks) if unfold else xs, H, 2, wg, hg)
        assert out.grad_fn.meta[-3:] == (False, False, True)      # (use16, usemc, use32)
        got = torch.autograd.grad(out, [xs, *wg, hg], dout.cuda())
    torch.cuda.synchronize()
    errs = [_rel64(a, r) for a, r in zip([out.detach(), *got], ref)]
    print(f"gru32 H=1024 layer unfold={unfold}: out {errs[0]:.3e} gradients {' '.join(f'{e:.3e}' for e in errs[1:])}")
    assert errs[0] < 1e-4, errs[0]
    for i, e in enumerate(errs[1:]):
        assert e < 2e-4, (i, e)
    assert Fn.gru_status_value() == 0


def test_full_finetune_step():
    """5. Trainer.train_step of a full fine-tune (the w2v encoder optimised, so the Trainer switches to bf16x3 with
    its default policy) on the smallest trainer-test configuration with a GRU of hidden size 1024: the layers take
    "gru32", the losses are finite, the replaying Trainer (1 eager + 2 graph steps) agrees with the eager-only one,
    and the status word stays 0."""
    from tests.helpers import CFG, build_model, batch_dict
    from wav2vec2forbrain_amd.datasets.batch_types import make_b2t_batch
    from wav2vec2forbrain_amd.train.train_loop import Trainer
    from wav2vec2forbrain_amd.workloads import SyntheticStepExperiment
    Fn = _fn()
    cfg = dict(CFG["plumbing_base"], gru_hidden=H)
    b = batch_dict(cfg)
    batch = make_b2t_batch(b["x"], b["target"], b["day_idxs"], b["input_lens"], b["target_lens"]).cuda()
    res = []
    for graphs in (False, True):
        model = build_model(cfg)
        model.train()
        with Fn.precision("bf16"):
            trainer = Trainer(SyntheticStepExperiment(model, unfreeze="brain_encoder+w2v", lr=1e-3, gradient_clipping=None))
            with trainer.precision_context():
                assert Fn._gru_recurrence(H) == "gru32"
            trainer.use_graphs = graphs
            trainer.capture_after = 1
            losses = [float(trainer.train_step(batch).metrics["ctc_loss"]) for _ in range(3)]
        torch.cuda.synchronize()
        if graphs:
            assert (trainer.eager_steps, trainer.graph_steps) == (1, 2)
        res.append(losses)
        trainer.release_graphs()
        Fn.set_deferred_wgrad([])
    print(f"gru32 H=1024 full fine-tune train_step losses: eager {res[0]} replayed {res[1]}")
    assert all(math.isfinite(v) for v in res[0] + res[1])
    np.testing.assert_allclose(res[1], res[0], rtol=1e-5, atol=0)
    assert Fn.gru_status_value() == 0
