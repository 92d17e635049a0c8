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
import functools
import math

import numpy as np
import pytest
import torch

from tests.helpers import CFG, load_fixture, build_model, batch_dict

pytestmark = pytest.mark.gpu

B, NH, DH = 2, 2, 64
D = NH * DH
SCALE = DH ** -0.5
ULP4 = 4 * 2.0 ** -24
SEED = 0x5EED1234


def _fn():
    from wav2vec2forbrain_amd import functional as Fn
    return Fn


@functools.lru_cache(maxsize=None)
def _inputs(T):
    g = torch.Generator().manual_seed(1000 + T)
    qkv = torch.randn(B * T, 3 * D, generator=g) * 0.5
    dO = torch.randn(B * T, D, generator=g)
    return qkv, dO


def _heads(x, T):   # (B*T, nh*dh) -> (B, nh, T, dh)
    return x.view(B, T, NH, DH).permute(0, 2, 1, 3)


def _ref64(T, keep=None, p=0.0):
    """float64 restatement: O (B*T, D), ln-domain lse (B, nh, T), dqkv (B*T, 3D); keep: (B, nh, T, T) bool."""
    qkv, dO = _inputs(T)
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = (_heads(x[:, i * D:(i + 1) * D], T) for i in range(3))
    S = q @ k.transpose(-1, -2) * SCALE
    lse = torch.logsumexp(S, -1)
    P = torch.softmax(S, -1)
    if keep is not None:
        P = P * keep.double() / (1.0 - p)
    O = (P @ v).permute(0, 2, 1, 3).reshape(B * T, D)
    O.backward(dO.double())
    return O.detach(), lse.detach(), x.grad.detach()


def _nan_bufs(T):
    nan = float("nan")
    return (torch.full((B * T, D), nan, device="cuda"), torch.full((B, NH, T), nan, device="cuda"),
            torch.full((B * T, 3 * D), nan, device="cuda"), torch.full((2, B, NH, T), nan, device="cuda"))


def _fused(T, p, seed=SEED, bufs=None):
    """O, lse2, dqkv, delta from the C entry points (into bufs when given)."""
    Fn = _fn()
    qkv, dO = (t.cuda() for t in _inputs(T))
    if bufs is None:
        bufs = _nan_bufs(T)
    O, lse2, dqkv, delta = bufs
    Fn._lib.call("b2p_attn32_long_fwd", qkv.data_ptr(), O.data_ptr(), lse2.data_ptr(), B, T, NH, DH, SCALE, p, seed,
                 Fn._st())
    Fn._lib.call("b2p_attn32_long_bwd", qkv.data_ptr(), dO.data_ptr(), lse2.data_ptr(), delta.data_ptr(),
                 dqkv.data_ptr(), B, T, NH, DH, SCALE, p, seed, Fn._st())
    torch.cuda.synchronize()
    return O, lse2, dqkv, delta


def _unfused(T, p, seed=SEED):
    """O, dqkv, P, Pd of the unfused fp32-mode path on the same inputs."""
    Fn = _fn()
    qkv, dO = (t.cuda() for t in _inputs(T))
    with Fn.precision("fp32"), Fn.fused_attn32(False):
        P, Pd, O = Fn._attn_core_fwd(qkv, B, T, NH, DH, p, seed)
        assert P.dim() == 4
        dqkv = Fn._attn_core_bwd(qkv, P, Pd, dO, B, T, NH, DH, p, seed)
    torch.cuda.synchronize()
    return O, dqkv, P[..., :T], (P if Pd is None else Pd)[..., :T]


def _err(x, ref):
    return float((x.detach().double().cpu() - ref).abs().max())


def _hold(what, T, got, unf, ref):
    e_f, e_u, m = _err(got, ref), (0.0 if unf is None else _err(unf, ref)), float(ref.abs().max())
    bound = 2 * e_u + ULP4 * m
    print(f"attn32_long T'={T} {what}: E_u {e_u:.3e} E_f {e_f:.3e} bound {bound:.3e} max|ref| {m:.3e}")
    return e_f <= bound, (what, T, e_f, e_u, bound)


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


def _dropout_case(T, p):
    Ou, du, P, Pd = _unfused(T, p)
    assert bool((P > 0).all())          # far above fp32 underflow: Pd != 0 is the keep pattern
    keep = (Pd != 0).cpu()
    frac = float(keep.float().mean())
    assert abs(frac - (1 - p)) < 0.05, frac
    Oref, _, dref = _ref64(T, keep, p)
    O, _, dqkv, _ = _fused(T, p)
    res = [_hold(f"O p={p}", T, O, Ou, Oref), _hold(f"dqkv p={p}", T, dqkv, du, dref)]
    assert all(ok for ok, _ in res), [r for ok, r in res if not ok]
    return O


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


def _batch(cfg):
    from wav2vec2forbrain_amd.datasets.batch_types import make_b2t_batch
    b = batch_dict(cfg)
    return make_b2t_batch(b["x"], b["target"], b["day_idxs"], b["input_lens"], b["target_lens"]).cuda()


def _attn_gemms(log, nz):
    return [e for e in log if e["nz"] == nz]


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
    """test_attn32_gpu.py::_three_steps at T' = 313: one eager step, then two more steps: replays of the captured
    step (graphs), or eager launches of the very step the capture records: the device-drawn LayerDrop form, the
    same host-drawn seeds and the same step counter mixed into every dropout seed. Tiny Conformer with head size
    64 in fp32 mode, the 0.1 training dropouts (attention dropout among them), LayerDrop 0.5, Adam over the brain
    encoder."""
    Fn = _fn()
    from wav2vec2forbrain_amd.optim import HipAdam
    from wav2vec2forbrain_amd.train.step_graph import StepGraph
    lib = Fn._lib.load()
    cfg = CONF_LONG
    model = build_model(cfg, train_dropouts=True)
    model.train()
    for m in model.modules():
        if hasattr(m, "sync_metrics"):
            m.sync_metrics = False
    model.w2v_encoder.wav2vec2_conformer.encoder.config.layerdrop = 0.5
    for n, q in model.named_parameters():
        if not n.startswith("brain_encoder."):
            q.requires_grad_(False)
    opt = HipAdam([q for q in model.brain_encoder.parameters()], lr=1e-3)
    batch = _batch(cfg)

    def fwd_bwd():
        opt.zero_grad()
        out = model(batch)
        out.loss.backward()
        return out.metrics["ctc_loss"]

    def step():
        loss = fwd_bwd()
        opt.step()
        return loss

    def reseed():     # the seeds the host draws while the step is captured: every replay reuses them
        Fn.SEEDS.reseed(900)
        Fn.LD_SEEDS.reseed(901)

    Fn.SEEDS.reseed(777)
    torch.manual_seed(779)      # the eager step's host LayerDrop draws
    epoch = torch.zeros(1, dtype=torch.int64, device="cuda")
    patterns = []
    try:
        Fn.ATTN32_MODES = (1, 3)    # the fused kernels in fp32 arithmetic (the fp32 mode's default is unfused)
        with Fn.precision("fp32"):
            losses = [float(step())]
            Fn.GEMM_LOG = []            # every layer runs below (LayerDrop gates them on the device)
            Fn.LAYERDROP_LOG = []
            if graphs:
                reseed()
                sg = StepGraph(step, opt, warmup=0, warm_replays=0, epoch=epoch)
                sg.capture()
                for _ in range(2):
                    losses.append(float(sg.replay()))
                    patterns.append(tuple(Fn.layerdrop_keep(0.5, s, int(epoch.item())) for s in Fn.LAYERDROP_LOG))
                sg.release()
            else:
                real = Fn.capturing
                try:
                    Fn._lib.check(lib.b2p_set_seed_epoch(ctypes.c_void_p(epoch.data_ptr())), "set_seed_epoch")
                    for _ in range(2):
                        reseed()
                        Fn.LAYERDROP_LOG = []
                        Fn._lib.check(lib.b2p_seed_epoch_step(ctypes.c_void_p(epoch.data_ptr()),
                                                              ctypes.c_void_p(Fn._st())), "step")
                        Fn.capturing = lambda: True      # the forward and backward the capture records
                        try:
                            loss = fwd_bwd()
                        finally:
                            Fn.capturing = real
                        opt.step()
                        losses.append(float(loss))
                        patterns.append(tuple(Fn.layerdrop_keep(0.5, s, int(epoch.item())) for s in Fn.LAYERDROP_LOG))
                finally:
                    Fn.capturing = real
                    Fn._lib.check(lib.b2p_set_seed_epoch(None), "set_seed_epoch")
            n_attn = len(_attn_gemms(Fn.GEMM_LOG, cfg["B"] * cfg["heads"]))
    finally:
        Fn.GEMM_LOG = None
        Fn.LAYERDROP_LOG = None
        Fn.ATTN32_MODES = (3,)
    torch.cuda.synchronize()
    opt.sync_steps()
    return losses, {n: q.detach().clone() for n, q in model.named_parameters()}, n_attn, patterns


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
