"""The activation table on the device: b2p_act_fwd / b2p_act_bwd for every id against float64 torch,
Fn.linear with a table activation against float64 autograd, the training step with each activation
against the reference's own modules (tests/golden/tiny_act.npz, made by make_golden_act.py), and the
step inside a captured Trainer.train_step."""
import functools

import numpy as np
import pytest
import torch

from tests import act_cases as AC
from tests.helpers import load_fixture

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 1028, 4099)


def _fn():
    from wav2vec2forbrain_amd import functional as Fn
    return Fn


@functools.lru_cache(maxsize=None)
def _points():
    """The grid with the extreme points first, so that every size >= 10 holds them."""
    g = AC.grid()
    return torch.cat([g[1024:], g[:1024]])


@functools.lru_cache(maxsize=None)
def _truth(act):
    return AC.truth(AC.ID_NAME[act], _points())


def _take(t, n):
    return t[torch.arange(n) % t.numel()]


def _buf(n, off):
    """n floats on the device starting `off` floats after a 16-byte boundary."""
    return torch.empty(n + 4, device="cuda")[off:off + n]


@pytest.mark.parametrize("act", range(AC.ID_LAST + 1), ids=[AC.ID_NAME[a] for a in range(AC.ID_LAST + 1)])
def test_kernels_against_float64(act):
    """Value and derivative of every id within 16 * 2^-24 * max(1, |truth|) of float64 torch on the
    1,024-point grid and at +-30 .. +-1e30: the 16-byte form (n % 4 == 0, aligned), the scalar form
    (other n, or a start one float off alignment), and in place. Where the truth overflows fp32 the
    result is that infinity; nothing is NaN. Measured maxima: profiles/r15a_act_errors.txt."""
    Fn = _fn()
    want_v, want_g = _truth(act)
    worst_v = worst_g = 0.0
    for n in SIZES:
        wv, wg = _take(want_v, n), _take(want_g, n)
        for off in (0, 1):
            x = _buf(n, off)
            x.copy_(_take(_points(), n))
            assert x.data_ptr() % 16 == 4 * off
            y = Fn.act_fwd(x, act, _buf(n, off))
            worst_v = max(worst_v, AC.err_ratio(y, wv))
            one = _buf(n, off).fill_(1.0)
            g = Fn._act_bwd(one, x, act, _buf(n, off))
            worst_g = max(worst_g, AC.err_ratio(g, wg))
            if n == 1028:
                # dy != 1: one fp32 multiply on top of the derivative
                dy = torch.linspace(-2.0, 3.0, n, device="cuda")
                dx = Fn._act_bwd(dy, x, act, _buf(n, off))
                assert torch.equal(dx, dy * g)
                # in place: out == pre
                xi = _buf(n, off).copy_(x)
                assert Fn.act_fwd(xi, act, xi) is xi and torch.equal(xi, y)
    print(f"{AC.ID_NAME[act]}: worst value error {worst_v / AC.BOUND:.3f} of the bound, derivative "
          f"{worst_g / AC.BOUND:.3f} (bound {AC.BOUND:.3e} * max(1, |truth|))")
    assert worst_v <= AC.BOUND, (AC.ID_NAME[act], worst_v)
    assert worst_g <= AC.BOUND, (AC.ID_NAME[act], worst_g)


@pytest.mark.parametrize("act", range(4), ids=[AC.ID_NAME[a] for a in range(4)])
def test_act_bwd_epilogue_ids_bit_identical(act):
    """Ids 0-3 through b2p_act_bwd keep the expressions they had before the table: bit-identical to the
    GEMM epilogue's act_bwd (csrc/gemm_epi.h, the same expressions, untouched), reached through an
    exact product: (dy @ I) * act'(pre) in fp32 mode adds only exact zeros to dy."""
    Fn = _fn()
    M, N = 58, 40
    torch.manual_seed(5)
    pre = _take(_points(), M * N).cuda().view(M, N).contiguous()
    dy = torch.randn(M, N, device="cuda")
    eye = torch.eye(N, device="cuda")
    want = torch.empty(M, N, device="cuda")
    with Fn.precision("fp32"):
        Fn.mm_nn(dy, eye, want, act_bwd=act, aux=pre if act else None)
    if act == 0:
        assert torch.equal(want, dy)
    for off in (0, 1):   # the 16-byte form and the scalar form
        got = Fn._act_bwd(_buf(M * N, off).copy_(dy.view(-1)), _buf(M * N, off).copy_(pre.view(-1)), act,
                          _buf(M * N, off))
        assert torch.equal(got.view(torch.int32), want.view(-1).view(torch.int32))


def test_unknown_id_is_an_error_on_the_device_path():
    Fn = _fn()
    x = torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError, match="99"):
        Fn.act_fwd(x, 99)
    with pytest.raises(RuntimeError, match="99"):
        Fn._act_bwd(x, x, 99)
    out = torch.empty(4, 4, device="cuda")
    with pytest.raises(ValueError, match="relu"):   # no caller hands gemm() a table id; it says so if one does
        Fn.mm_nt(out, out, out, act=AC.IDS["relu"])


@pytest.mark.parametrize("act", AC.NEW_IDS, ids=[AC.ID_NAME[a] for a in AC.NEW_IDS])
def test_linear_with_table_activation(act):
    """Fn.linear(x, W, b, act) (GEMM + b2p_act_fwd, backward through b2p_act_bwd) in fp32 mode against
    float64 autograd, at the tolerance tests/test_gemm_gpu.py::test_epilogue applies to its fp32-mode
    gelu epilogue (2e-5 of the scale)."""
    Fn = _fn()
    M, K, N = 58, 32, 40
    torch.manual_seed(11)
    x = torch.randn(M, K, device="cuda", requires_grad=True)
    W = (torch.randn(N, K, device="cuda") / 4).requires_grad_(True)
    b = torch.randn(N, device="cuda", requires_grad=True)
    G = torch.randn(M, N, device="cuda")
    with Fn.precision("fp32"):
        out = Fn.linear(x, W, b, act)
        dx, dW, db = torch.autograd.grad(out, (x, W, b), G)
        with torch.no_grad():   # eval: the activation is applied in place, one buffer
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out_ng = Fn.linear(x, W, b, act)
            peak = torch.cuda.max_memory_allocated() - base
    assert torch.equal(out_ng, out)
    assert peak < 2 * out.numel() * 4, peak
    x64, W64, b64 = (t.detach().double().cpu().requires_grad_(True) for t in (x, W, b))
    pre = x64 @ W64.t() + b64
    ref = AC.FN[AC.ID_NAME[act]](pre)
    rx, rW, rb = torch.autograd.grad(ref, (x64, W64, b64), G.double().cpu())
    tol = 2e-5
    out_scale = max(float(pre.detach().abs().max()), float(ref.detach().abs().max()))
    for name, got, want, scale in (("out", out, ref, out_scale),
                                   ("dx", dx, rx, float(rx.abs().max())), ("dW", dW, rW, float(rW.abs().max())),
                                   ("db", db, rb, float(rb.abs().max()))):
        err = float((got.detach().double().cpu() - want.detach()).abs().max())
        print(f"{AC.ID_NAME[act]} {name}: max err {err:.3e} of scale {scale:.3e}")
        assert err <= tol * (scale + 1e-6), (name, err, scale)


# ------------------------------------------------------------------ model against the reference
MODEL_NAMES = ["relu", "relu2", "relu6", "tanh", "sigmoid", "mish", "quick_gelu", "laplace", "gelu_new", "gelu_10",
               "linear"]
# a derivative that jumps: 16-bit noise in the pre-activation flips the gate of the few elements nearest
# the kink (about 4 of ~2,300 lie within bf16 noise of 0: a relative L2 of order 4e-2 on the fc weight
# gradient, which the reference's own arithmetic at 16 bits would show too). Their backward is the same
# fp32 elementwise kernel in every mode, pinned by test_kernels_against_float64.
DERIVATIVE_JUMPS = ("relu", "relu6")


@functools.lru_cache(maxsize=None)
def _fixture():
    return load_fixture("tiny_act")


def _step(name, mode):
    from wav2vec2forbrain_amd.datasets.batch_types import make_b2t_batch
    from wav2vec2forbrain_amd.workloads import build_model, tiny_act_config
    Fn = _fn()
    fx = _fixture()
    model = build_model(tiny_act_config(name))
    model.train()
    batch = make_b2t_batch(torch.from_numpy(fx["x"]), torch.from_numpy(fx["target"]), torch.from_numpy(fx["day_idxs"]),
                           torch.from_numpy(fx["input_lens"]), torch.from_numpy(fx["target_lens"])).cuda()
    with Fn.precision(mode):
        out = model(batch)
        out.loss.backward()
    torch.cuda.synchronize()
    return model, out


@pytest.mark.parametrize("name,mode", [(n, m) for m in ("fp32", "bf16") for n in MODEL_NAMES] +
                         [("relu", "bf16x3"), ("mish", "bf16x3")])
def test_step_matches_reference(name, mode):
    """One deterministic training step of the tiny_act workload vs the reference's own modules with
    encoder_fc_activation_function=name, at the gates tests/test_model_gpu.py holds its tiny fixtures to:
    fp32 (and bf16x3) loss 2e-5, logits 2e-4 of max, gradients 2e-3; bf16 loss 1e-3, logits 2e-2 relative
    L2, gradients 2.5e-2 (not for relu / relu6, see DERIVATIVE_JUMPS). bf16x3 checks loss and logits."""
    fx = _fixture()
    assert list(fx["names"]) == MODEL_NAMES
    model, out = _step(name, mode)
    exact = mode != "bf16"
    ref = float(fx[f"{name}/loss"])
    got = out.metrics["ctc_loss"]
    lg, rl = out.logits.detach().cpu().numpy(), fx[f"{name}/logits"]
    print(f"{name} [{mode}]: loss rel err {abs(got - ref) / abs(ref):.3e}, logits max err / max "
          f"{np.abs(lg - rl).max() / np.abs(rl).max():.3e}, rel L2 {np.linalg.norm(lg - rl) / np.linalg.norm(rl):.3e}")
    assert abs(got - ref) <= (2e-5 if exact else 1e-3) * abs(ref), (got, ref)
    if exact:
        np.testing.assert_allclose(lg, rl, rtol=0, atol=2e-4 * np.abs(rl).max())
    else:
        assert np.linalg.norm(lg - rl) <= 2e-2 * np.linalg.norm(rl)
    if mode == "bf16x3" or (mode == "bf16" and name in DERIVATIVE_JUMPS):
        return
    gtol = 2e-3 if mode == "fp32" else 2.5e-2
    names = list(fx["param_names"])
    gmax = max(float(fx[f"{name}/gnorm/{n}"]) for n in names)
    params = dict(model.named_parameters())
    assert set(names) == set(params)
    worst_norm = worst_l2 = 0.0
    full = 0
    for n in names:
        p = params[n]
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        ref_norm = float(fx[f"{name}/gnorm/{n}"])
        gn = float(g.double().norm())
        if ref_norm >= 1e-6 * gmax:
            worst_norm = max(worst_norm, abs(gn - ref_norm) / ref_norm)
        assert abs(gn - ref_norm) <= gtol * ref_norm + 1e-4 * gmax, (n, gn, ref_norm)
        if f"{name}/grad/{n}" not in fx:
            continue
        full += 1
        r, v = fx[f"{name}/grad/{n}"], g.cpu().numpy()
        if mode == "fp32":
            scale = max(np.abs(r).max(), 1e-3 * gmax)
            assert np.abs(v - r).max() <= gtol * scale + 1e-5 * gmax, n
        elif ref_norm < 1e-6 * gmax:
            assert np.linalg.norm(v) <= 1e-4 * gmax, n
        else:
            worst_l2 = max(worst_l2, float(np.linalg.norm(v - r) / max(np.linalg.norm(r), 1e-30)))
            assert np.linalg.norm(v - r) <= gtol * np.linalg.norm(r) + 1e-5 * gmax, n
    assert full == 4   # fc.0 / fc.2 weight and bias
    print(f"{name} [{mode}]: worst gradient-norm error {worst_norm:.3e}, worst fc-gradient relL2 {worst_l2:.3e} "
          f"(gate {gtol:g})")


def test_captured_step_matches_eager():
    """Trainer.train_step on tiny_act with relu: after the eager first step, three replayed steps give the
    losses and the brain-encoder parameters of eager steps, at the tolerance tests/test_trainer_gpu.py
    applies to its replay-vs-eager comparison (the new launch captures: current stream, no allocation
    beyond _Linear's, nothing read back)."""
    from wav2vec2forbrain_amd.datasets.batch_types import make_b2t_batch
    from wav2vec2forbrain_amd.train.train_loop import Trainer
    from wav2vec2forbrain_amd.workloads import SyntheticStepExperiment, build_model, tiny_act_config
    Fn = _fn()
    fx = _fixture()
    batch = make_b2t_batch(torch.from_numpy(fx["x"]), torch.from_numpy(fx["target"]), torch.from_numpy(fx["day_idxs"]),
                           torch.from_numpy(fx["input_lens"]), torch.from_numpy(fx["target_lens"])).cuda()
    res = []
    for graphs in (False, True):
        model = build_model(tiny_act_config("relu"))
        model.train()
        with Fn.precision("bf16"):
            trainer = Trainer(SyntheticStepExperiment(model, lr=1e-3))
            trainer.use_graphs = graphs
            trainer.capture_after = 1
            losses = [float(trainer.train_step(batch).metrics["ctc_loss"]) for _ in range(4)]
        torch.cuda.synchronize()
        if graphs:
            assert (trainer.eager_steps, trainer.graph_steps) == (1, 3)
        trainer.optimizer.sync_steps()
        res.append((losses, {n: p.detach().clone() for n, p in model.named_parameters()
                             if n.startswith("brain_encoder.")}))
        trainer.release_graphs()
        Fn.set_deferred_wgrad([])
    (la, pa), (lb, pb) = res
    assert la[0] != la[3]   # the steps moved the parameters
    np.testing.assert_allclose(lb, la, rtol=1e-5, atol=0)
    assert pa
    for n in pa:
        assert float((pa[n] - pb[n]).norm()) <= 1e-5 * float(pa[n].norm()) + 1e-7, n
