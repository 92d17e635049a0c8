"""The 16-bit layer backwards without their fp32 gradient images (functional._GRAD_IMG32 False, the
default) against the same backwards with them (_GRAD_IMG32 True: the LayerNorm backwards write dxd, the
attention backward writes the fp32 dqkv and the Q/K/V bias gradients are its column sums).

A tiny post-LN layer (D 128, two heads of 64, F 256, B 2, T 40) and a tiny Conformer attention block:
every gradient except bq / bk / bv is bitwise equal between the two paths; bq / bk / bv are, on either
path, an fp32 summation in some order of the n = B * T values of their dqkv column, so each lies within
n * 2^-24 * sum|x| of the column's float64 sum (x: the fp32 image, captured from the old path's
_attn16_bwd call). Trained biases are checked as returned gradients; frozen (deferred) ones in .grad after
join_wgrad, also after a second backward that accumulates: .grad is then an fp32 summation of the 2n values
of two identical images, bound 2n * 2^-24 * 2 sum|x|.

A captured-and-replayed Trainer step against its eager twin (as tests/test_trainer_gpu.py; on plumbing_base,
whose 64-wide heads take the fused attention, which the tiny golden configurations' 16-wide heads never do)
catches a partial buffer that a replay does not rewrite."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, D, NH, FF = 2, 40, 128, 2, 256
N = B * T
U = 2.0 ** -24
BIAS_QKV = (1, 3, 5)   # positions of bq, bk, bv among the post-LN layer's parameters


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def _capture_image(Fn, monkeypatch, store):
    """The old path's fp32 dqkv image, taken from the _attn16_bwd call inside the layer backward."""
    real = Fn._attn16_bwd

    def spy(*a, **k):
        out = real(*a, **k)
        if out[0] is not None:
            store.append(out[0].detach().clone())
        return out

    monkeypatch.setattr(Fn, "_attn16_bwd", spy)


def _check_bias(got, image, q, terms, label):
    x = image[:, q * D:(q + 1) * D].double()
    k = terms // N                      # images accumulated
    ref, mag = k * x.sum(0), k * x.abs().sum(0)
    err = (got.double().reshape(-1) - ref).abs()
    bound = terms * U * mag
    worst = float((err / bound.clamp(min=1e-300)).max())
    print(f"{label}: max err/bound {worst:.3e}")
    assert bool((err <= bound).all()), (label, worst)
    assert float(mag.min()) > 0, label


def _layer_params(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(D, D), (D,), (D, D), (D,), (D, D), (D,), (D, D), (D,), (D,), (D,), (FF, D), (FF,), (D, FF), (D,), (D,), (D,)]
    ps = [(torch.randn(*s, generator=g) / math.sqrt(s[-1])).cuda() for s in shapes]
    ps[8] = torch.ones(D, device="cuda")
    ps[14] = torch.ones(D, device="cuda")
    x = torch.randn(B, T, D, generator=g).cuda()
    dy = torch.randn(B, T, D, generator=g).cuda()
    return ps, x, dy


def _conf_params(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(D,), (D,), (D, D), (D,), (D, D), (D,), (D, D), (D,), (D, D), (D,)]   # g, b, wq, bq, wk, bk, wv, bv, wo, bo
    ps = [(torch.randn(*s, generator=g) / math.sqrt(s[-1])).cuda() for s in shapes]
    ps[0] = torch.ones(D, device="cuda")
    x = torch.randn(B, T, D, generator=g).cuda()
    dy = torch.randn(B, T, D, generator=g).cuda()
    return ps, x, dy


def _apply_layer(Fn, xg, pg):
    return Fn._EncoderLayer16.apply(xg, (NH, 1e-5, 0.1, 0.1, 0.1, (31, 32, 33, 34)), *pg)


def _apply_conf(Fn, xg, pg):
    return Fn._ConformerAttnBlock.apply(xg, *pg, None, None, (NH, 1e-5, 0.1, 0.1, (51, 52)))


CASES = {"post_ln": (_layer_params, _apply_layer, BIAS_QKV), "conformer": (_conf_params, _apply_conf, (3, 5, 7))}


def _run(Fn, kind, f16, frozen, old, passes=1):
    """Gradients of one block on the old or new path. frozen: every parameter is a deferred frozen one (its
    gradient arrives in .grad after join_wgrad), else all are returned by autograd."""
    make, apply, _ = CASES[kind]
    ps, x, dy = make(7)
    Fn._GRAD_IMG32[0] = old
    try:
        with Fn.precision("bf16"), Fn.forward_f16(f16):
            pg = [torch.nn.Parameter(p.clone()) for p in ps]
            xg = x.clone().requires_grad_(True)
            if frozen:
                Fn.set_deferred_wgrad(pg)
            dx = None
            for _ in range(passes):
                out = apply(Fn, xg, pg)
                got = torch.autograd.grad(out, [xg] + pg, dy, allow_unused=True)
                dx = got[0]
                if frozen:
                    assert all(g is None for g in got[1:])
                    Fn.join_wgrad()
            torch.cuda.synchronize()
            grads = [p.grad.detach().clone() for p in pg] if frozen else [g.detach().clone() for g in got[1:]]
    finally:
        Fn._GRAD_IMG32[0] = False
        Fn.set_deferred_wgrad([])
    return out.detach().clone(), dx.detach().clone(), grads


@pytest.mark.parametrize("frozen", [False, True], ids=["trained", "frozen"])
@pytest.mark.parametrize("kind,f16", [("post_ln", False), ("post_ln", True), ("conformer", True)])
def test_block_gradients_without_fp32_images(kind, f16, frozen, monkeypatch):
    from wav2vec2forbrain_amd import functional as Fn
    images = []
    _capture_image(Fn, monkeypatch, images)
    qkv_b = CASES[kind][2]
    for passes in ((1, 2) if frozen else (1,)):
        del images[:]
        out_o, dx_o, g_o = _run(Fn, kind, f16, frozen, True, passes)
        assert len(images) == passes            # the old path wrote the image, once per backward
        image = images[0]
        out_n, dx_n, g_n = _run(Fn, kind, f16, frozen, False, passes)
        assert len(images) == passes            # the new path wrote none
        assert _bits(out_o, out_n) and _bits(dx_o, dx_n)
        assert len(g_o) == len(g_n)
        for i, (a, b) in enumerate(zip(g_o, g_n)):
            if i in qkv_b:
                q = qkv_b.index(i)
                _check_bias(a, image, q, passes * N, f"{kind} f16={f16} frozen={frozen} passes={passes} old b{'qkv'[q]}")
                _check_bias(b, image, q, passes * N, f"{kind} f16={f16} frozen={frozen} passes={passes} new b{'qkv'[q]}")
            else:
                assert _bits(a, b), (kind, f16, frozen, passes, i)


def test_layernorm_backwards_allocate_no_image():
    """_EncoderLayer16.backward asks both LayerNorm backwards for the form without dxd."""
    from wav2vec2forbrain_amd import functional as Fn
    seen = []
    real = Fn._ln_bwd16

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append((k.get("want_dxd", True), out[3] is None))
        return out

    Fn._ln_bwd16 = spy
    try:
        _run(Fn, "post_ln", True, False, False)
    finally:
        Fn._ln_bwd16 = real
    assert seen == [(False, True), (False, True)], seen


def test_trainer_replay_matches_eager_without_images():
    from tests.helpers import CFG, build_model, batch_dict
    from wav2vec2forbrain_amd import functional as Fn
    from wav2vec2forbrain_amd.datasets.batch_types import make_b2t_batch
    from wav2vec2forbrain_amd.train.train_loop import Trainer
    from wav2vec2forbrain_amd.workloads import SyntheticStepExperiment
    cfg = CFG["plumbing_base"]
    b = batch_dict(cfg)
    full = make_b2t_batch(b["x"], b["target"], b["day_idxs"], b["input_lens"], b["target_lens"]).cuda()
    flip = make_b2t_batch(b["x"].flip(0).contiguous(), b["target"].flip(0).contiguous(), b["day_idxs"].flip(0),
                          b["input_lens"].flip(0), b["target_lens"].flip(0)).cuda()
    res = []
    for graphs in (False, True):
        model = build_model(cfg)
        model.train()
        with Fn.precision("bf16"):
            trainer = Trainer(SyntheticStepExperiment(model, lr=1e-3, gradient_clipping=None))
            trainer.use_graphs = graphs
            trainer.capture_after = 1
            losses = [float(trainer.train_step(batch).metrics["ctc_loss"]) for batch in (full, flip, full)]
        torch.cuda.synchronize()
        if graphs:
            assert (trainer.eager_steps, trainer.graph_steps) == (1, 2)
        trainer.optimizer.sync_steps()
        res.append((losses, {n: p.grad.detach().clone() for n, p in model.named_parameters()
                             if not n.startswith("brain_encoder.") and p.grad is not None}))
        trainer.release_graphs()
        Fn.set_deferred_wgrad([])
    (la, fa), (lb, fb) = res
    np.testing.assert_allclose(lb, la, rtol=1e-5, atol=0)
    assert set(fa) == set(fb)
    biases = [n for n in fa if n.endswith(("q_proj.bias", "k_proj.bias", "v_proj.bias"))]
    assert len(biases) == 3 * cfg["layers"], biases
    for n in fa:   # the frozen gradients (the Q/K/V biases' partial sums among them) accumulate across replays
        assert float((fa[n] - fb[n]).norm()) <= 1e-5 * float(fa[n].norm()) + 1e-7, n
