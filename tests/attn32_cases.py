"""What tests/test_attn32_gpu.py and tests/test_attn32_long_gpu.py share: the inputs, the float64 restatement, the
fused and unfused runs and the bound of the kernel cases, for one shape class of csrc/attn32.hip (its forward and
backward entry points and the tag its figures are printed under), and the three-step capture comparison.

Every kernel case uses head size 64, B = 2, heads = 2 (batch and head strides both exercised), qkv = randn * 0.5
and dO = randn from a generator seeded 1000 + T'. The rule (the test modules' docstrings say why):

    E_f <= 2 * E_u + 4 * 2**-24 * max|ref|     (max abs errors against float64, per output)
"""
import ctypes
import functools

import torch

from tests.helpers import build_model, batch_dict

B, NH, DH = 2, 2, 64
D = NH * DH
SCALE = DH ** -0.5
ULP4 = 4 * 2.0 ** -24
SEED = 0x5EED1234


def fn():
    from wav2vec2forbrain_amd import functional as Fn
    return Fn


@functools.lru_cache(maxsize=None)
def inputs(T):
    g = torch.Generator().manual_seed(1000 + T)
    qkv = torch.randn(B * T, 3 * D, generator=g) * 0.5
    dO = torch.randn(B * T, D, generator=g)
    return qkv, dO


def _heads(x, T):   # (B*T, nh*dh) -> (B, nh, T, dh)
    return x.view(B, T, NH, DH).permute(0, 2, 1, 3)


def ref64(T, keep=None, p=0.0):
    """float64 restatement: O (B*T, D), ln-domain lse (B, nh, T), dqkv (B*T, 3D); keep: (B, nh, T, T) bool."""
    qkv, dO = inputs(T)
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


@functools.lru_cache(maxsize=None)
def ref64_plain(T):
    return ref64(T)


def nan_bufs(T):
    nan = float("nan")
    return (torch.full((B * T, D), nan, device="cuda"), torch.full((B, NH, T), nan, device="cuda"),
            torch.full((B * T, 3 * D), nan, device="cuda"), torch.full((2, B, NH, T), nan, device="cuda"))


def unfused(T, p, seed=SEED):
    """O, dqkv, P, Pd of the unfused fp32-mode path on the same inputs."""
    Fn = fn()
    qkv, dO = (t.cuda() for t in inputs(T))
    with Fn.precision("fp32"), Fn.fused_attn32(False):
        P, Pd, O = Fn._attn_core_fwd(qkv, B, T, NH, DH, p, seed)
        assert P.dim() == 4
        dqkv = Fn._attn_core_bwd(qkv, P, Pd, dO, B, T, NH, DH, p, seed)
    torch.cuda.synchronize()
    return O, dqkv, P[..., :T], (P if Pd is None else Pd)[..., :T]


def _err(x, ref):
    return float((x.detach().double().cpu() - ref).abs().max())


class Attn32Cases:
    """The kernel cases of one shape class: fwd / bwd are its C entry points, tag prefixes the printed figures."""

    def __init__(self, fwd, bwd, tag):
        self.fwd, self.bwd, self.tag = fwd, bwd, tag

    def fused(self, T, p, seed=SEED, bufs=None):
        """O, lse2, dqkv, delta from the C entry points (into bufs when given)."""
        Fn = fn()
        qkv, dO = (t.cuda() for t in inputs(T))
        if bufs is None:
            bufs = nan_bufs(T)
        O, lse2, dqkv, delta = bufs
        Fn._lib.call(self.fwd, qkv.data_ptr(), O.data_ptr(), lse2.data_ptr(), B, T, NH, DH, SCALE, p, seed, Fn._st())
        Fn._lib.call(self.bwd, qkv.data_ptr(), dO.data_ptr(), lse2.data_ptr(), delta.data_ptr(), dqkv.data_ptr(),
                     B, T, NH, DH, SCALE, p, seed, Fn._st())
        torch.cuda.synchronize()
        return O, lse2, dqkv, delta

    def hold(self, what, T, got, unf, ref):
        e_f, e_u, m = _err(got, ref), (0.0 if unf is None else _err(unf, ref)), float(ref.abs().max())
        bound = 2 * e_u + ULP4 * m
        print(f"{self.tag} T'={T} {what}: E_u {e_u:.3e} E_f {e_f:.3e} bound {bound:.3e} max|ref| {m:.3e}")
        return e_f <= bound, (what, T, e_f, e_u, bound)

    def dropout_case(self, T, p):
        Ou, du, P, Pd = unfused(T, p)
        assert bool((P > 0).all())          # far above fp32 underflow: Pd != 0 is the keep pattern
        keep = (Pd != 0).cpu()
        frac = float(keep.float().mean())
        assert abs(frac - (1 - p)) < 0.05, frac
        Oref, _, dref = ref64(T, keep, p)
        O, _, dqkv, _ = self.fused(T, p)
        res = [self.hold(f"O p={p}", T, O, Ou, Oref), self.hold(f"dqkv p={p}", T, dqkv, du, dref)]
        assert all(ok for ok, _ in res), [r for ok, r in res if not ok]
        return O


def batch(cfg):
    from wav2vec2forbrain_amd.datasets.batch_types import make_b2t_batch
    b = batch_dict(cfg)
    return make_b2t_batch(b["x"], b["target"], b["day_idxs"], b["input_lens"], b["target_lens"]).cuda()


def attn_gemms(log, nz):
    return [e for e in log if e["nz"] == nz]


def three_steps(cfg, graphs):
    """One eager step, then two more steps: replays of the captured step (graphs), or eager launches of the very
    step the capture records: the device-drawn LayerDrop form, the same host-drawn seeds and the same step
    counter mixed into every dropout seed. cfg: a tiny Conformer with head size 64; fp32 mode, the 0.1 training
    dropouts (attention dropout among them), LayerDrop 0.5, Adam over the brain encoder."""
    Fn = fn()
    from wav2vec2forbrain_amd.optim import HipAdam
    from wav2vec2forbrain_amd.train.step_graph import StepGraph
    lib = Fn._lib.load()
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
    bt = batch(cfg)

    def fwd_bwd():
        opt.zero_grad()
        out = model(bt)
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
            n_attn = len(attn_gemms(Fn.GEMM_LOG, cfg["B"] * cfg["heads"]))
    finally:
        Fn.GEMM_LOG = None
        Fn.LAYERDROP_LOG = None
        Fn.ATTN32_MODES = (3,)
    torch.cuda.synchronize()
    opt.sync_steps()
    return losses, {n: q.detach().clone() for n, q in model.named_parameters()}, n_attn, patterns
