"""LayerDrop's select, route and flag launches folded into the layer's own kernels (functional._LD_FUSE).

Kernel level: the gate-aware LayerNorm entry points (b2p_layernorm_bwd_gated, b2p_layernorm_fwd16_sel,
b2p_layernorm_fwd_x16_sel) against the ungated calls on the tensors the route / select kernels would
have produced, and the one-launch flags (b2p_layerdrop_flags) against the host draw. Layer level: a
3-layer post-LN encoder (bf16 on the fused attention path, forward_f16 off and on, and fp32), captured
and replayed with the fold on and off. Every comparison is bitwise."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (1, 37, 300)     # 16 rows per backward block, 4 per forward block: one block, partial blocks, many
COLS = (4, 768)         # the smallest row the LayerNorm kernels accept (one float4), and the base width
GATES = ("open", "closed", "null")


def _fn():
    from wav2vec2forbrain_amd import functional as Fn
    return Fn


def _call(name, *args):
    from wav2vec2forbrain_amd import _lib
    _lib.call(name, *args, _lib.stream_ptr())


def P(t):
    return None if t is None else t.data_ptr()


def _gate(kind):
    return None if kind == "null" else torch.tensor([1 if kind == "open" else 0], dtype=torch.int32, device="cuda")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ln_inputs(rows, cols, seed=0):
    g = torch.Generator().manual_seed(1000 * rows + cols + seed)
    x = torch.randn(rows, cols, generator=g) * 1.5 + 0.3
    dy = torch.randn(rows, cols, generator=g)
    gamma = torch.randn(cols, generator=g)
    mean = x.mean(1)
    rstd = (x.var(1, unbiased=False) + 1e-5).rsqrt()
    acc = torch.randn(rows, cols, generator=g)
    return [t.cuda() for t in (x, dy, gamma, mean, rstd, acc)]


def _ln_bwd(x, dy, gamma, mean, rstd, acc2=None, dy_gate=None, acc2_gate=None, gated=False):
    """(dx, dx_dropped, d16, dgamma, dbeta, dbias_in) of one LayerNorm backward with the in-dropout on
    (the post-LN layer's form), through b2p_layernorm_bwd_gated or (gated=False) b2p_layernorm_bwd_acc2."""
    from wav2vec2forbrain_amd import _lib
    rows, cols = x.shape
    dx, dxd = torch.empty_like(x), torch.empty_like(x)
    d16 = torch.empty(rows, cols, device="cuda", dtype=torch.bfloat16)
    dg, db, dbi = (torch.empty(cols, device="cuda") for _ in range(3))
    ws = torch.empty(int(_lib.load().b2p_layernorm_bwd_workspace(rows, cols)), device="cuda")
    head = (P(dy), P(x), P(gamma), P(mean), P(rstd), P(dx), P(dg), P(db), rows, cols, None, P(acc2), 0.0, 0, P(dxd),
            0.1, 777, P(dbi), P(d16))
    if gated:
        _call("b2p_layernorm_bwd_gated", *head, P(dy_gate), P(acc2_gate), P(ws))
    else:
        _call("b2p_layernorm_bwd_acc2", *head, P(ws))
    torch.cuda.synchronize()
    return dx, dxd, d16, dg, db, dbi


@pytest.mark.parametrize("rows,cols", list(itertools.product(ROWS, COLS)))
def test_ln_bwd_gated_dy(rows, cols):
    """An open or null dy_gate is today's call; a closed one is today's call on dy = zeros, and dy is not
    read (it holds NaN in the gated call)."""
    x, dy, gamma, mean, rstd, _ = _ln_inputs(rows, cols)
    ref_open = _ln_bwd(x, dy, gamma, mean, rstd)
    ref_zero = _ln_bwd(x, torch.zeros_like(dy), gamma, mean, rstd)
    for kind in GATES:
        closed = kind == "closed"
        got = _ln_bwd(x, torch.full_like(dy, float("nan")) if closed else dy, gamma, mean, rstd,
                      dy_gate=_gate(kind), gated=True)
        for k, (a, b) in enumerate(zip(got, ref_zero if closed else ref_open)):
            assert _same(a, b), (kind, k)


@pytest.mark.parametrize("rows,cols", list(itertools.product(ROWS, COLS)))
def test_ln_bwd_gated_accum2(rows, cols):
    """dx_accum2 under acc2_gate: closed (or no gate) adds the tensor, open adds +0 without reading it."""
    x, dy, gamma, mean, rstd, acc = _ln_inputs(rows, cols, seed=1)
    ref_acc = _ln_bwd(x, dy, gamma, mean, rstd, acc2=acc)
    ref_zero = _ln_bwd(x, dy, gamma, mean, rstd, acc2=torch.zeros_like(acc))
    for kind in GATES:
        opened = kind == "open"
        got = _ln_bwd(x, dy, gamma, mean, rstd, acc2=torch.full_like(acc, float("nan")) if opened else acc,
                      acc2_gate=_gate(kind), gated=True)
        for k, (a, b) in enumerate(zip(got, ref_zero if opened else ref_acc)):
            assert _same(a, b), (kind, k)


@pytest.mark.parametrize("rows,cols", [(37, 4), (37, 768)])
def test_ln_bwd_gated_accum2_negative_zero(rows, cols):
    """The add is always performed: where the ungated sum is -0.0 (a -0.0 input gradient plus a -0.0 skip
    gradient), the closed gate keeps -0.0, and the open gate gives the +0.0 that adding the routed zeros
    gave. A skipped layer's LN1 backward sees exactly this: dy = 0 and negative gamma entries."""
    x, _, gamma, mean, rstd, _ = _ln_inputs(rows, cols, seed=2)
    dy = torch.zeros_like(x)
    gamma = -gamma.abs() - 0.1
    acc = torch.full_like(x, -0.0)
    ref_acc = _ln_bwd(x, dy, gamma, mean, rstd, acc2=acc)
    ref_zero = _ln_bwd(x, dy, gamma, mean, rstd, acc2=torch.zeros_like(acc))
    neg0 = torch.signbit(ref_acc[0]) & (ref_acc[0] == 0)
    assert bool(neg0.any()), "the case must contain a -0.0 sum"
    assert not bool((torch.signbit(ref_zero[0]) & (ref_zero[0] == 0)).any())
    closed = _ln_bwd(x, dy, gamma, mean, rstd, acc2=acc, acc2_gate=_gate("closed"), gated=True)
    opened = _ln_bwd(x, dy, gamma, mean, rstd, acc2=acc, acc2_gate=_gate("open"), gated=True)
    for k in range(6):
        assert _same(closed[k], ref_acc[k]), k
        assert _same(opened[k], ref_zero[k]), k


def _skip_sources(rows, cols):
    g = torch.Generator().manual_seed(5 * rows + cols)
    skip = torch.randn(rows, cols, generator=g).cuda()
    # 16-bit images that are NOT the rounding of skip: a closed gate must copy them, not repack
    s16 = torch.randn(rows, cols, generator=g).cuda().bfloat16()
    sh = torch.randn(rows, cols, generator=g).cuda().half()
    return skip, s16, sh


@pytest.mark.parametrize("rows,cols", list(itertools.product(ROWS, COLS)))
def test_ln_fwd16_select(rows, cols):
    """b2p_layernorm_fwd16_sel (the bf16 layer's last LayerNorm): open / null equals b2p_layernorm_fwd16;
    closed writes the skip sources (the bf16 image copied, or packed from skip when absent) and leaves the
    statistics those of x."""
    x, _, gamma, _, _, beta2 = _ln_inputs(rows, cols, seed=3)
    beta = beta2[0].contiguous()
    skip, s16, _ = _skip_sources(rows, cols)

    def run(gate=None, sk=None, sk16=None, sel=True):
        y = torch.empty_like(x)
        y16 = torch.empty(rows, cols, device="cuda", dtype=torch.bfloat16)
        mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
        head = (P(x), P(gamma), P(beta), P(y), P(y16), P(mean), P(rstd), rows, cols, 1e-5, 0.0, 0)
        if sel:
            _call("b2p_layernorm_fwd16_sel", *head, P(gate), P(sk), P(sk16))
        else:
            _call("b2p_layernorm_fwd16", *head)
        torch.cuda.synchronize()
        return y, y16, mean, rstd

    ref = run(sel=False)
    for kind in ("open", "null"):
        got = run(_gate(kind), skip, s16)
        assert all(_same(a, b) for a, b in zip(got, ref)), kind
    y, y16, mean, rstd = run(_gate("closed"), skip, s16)
    assert _same(y, skip) and _same(y16, s16) and _same(mean, ref[2]) and _same(rstd, ref[3])
    y, y16, mean, rstd = run(_gate("closed"), skip, None)
    assert _same(y, skip) and _same(y16, skip.bfloat16()) and _same(mean, ref[2]) and _same(rstd, ref[3])


@pytest.mark.parametrize("rows,cols", list(itertools.product(ROWS, COLS)))
def test_ln_fwd_x16_select(rows, cols):
    """b2p_layernorm_fwd_x16_sel (the forward_f16 layer's last LayerNorm: fp32 y, fp16 y16, bf16 y16b)."""
    x, _, gamma, _, _, beta2 = _ln_inputs(rows, cols, seed=4)
    beta = beta2[0].contiguous()
    skip, s16, sh = _skip_sources(rows, cols)

    def run(gate=None, sk=None, skh=None, sk16=None, sel=True):
        y = torch.empty_like(x)
        yh = torch.empty(rows, cols, device="cuda", dtype=torch.float16)
        yb = torch.empty(rows, cols, device="cuda", dtype=torch.bfloat16)
        mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
        head = (P(x), P(gamma), P(beta), P(y), P(yh), 1, P(yb), P(mean), P(rstd), rows, cols, 1e-5)
        if sel:
            _call("b2p_layernorm_fwd_x16_sel", *head, P(gate), P(sk), P(skh), P(sk16))
        else:
            _call("b2p_layernorm_fwd_x16", *head)
        torch.cuda.synchronize()
        return y, yh, yb, mean, rstd

    ref = run(sel=False)
    for kind in ("open", "null"):
        got = run(_gate(kind), skip, sh, s16)
        assert all(_same(a, b) for a, b in zip(got, ref)), kind
    y, yh, yb, mean, rstd = run(_gate("closed"), skip, sh, s16)
    assert _same(y, skip) and _same(yh, sh) and _same(yb, s16) and _same(mean, ref[3]) and _same(rstd, ref[4])
    y, yh, yb, mean, rstd = run(_gate("closed"), skip, None, None)
    assert _same(y, skip) and _same(yh, skip.half()) and _same(yb, skip.bfloat16())
    assert _same(mean, ref[3]) and _same(rstd, ref[4])


@pytest.mark.parametrize("n", [1, 12, 32, 45])
def test_one_launch_flags_match_host_draw(n):
    """b2p_layerdrop_flags (45 layers: past the 32 seeds one launch carries) against layerdrop_keep for
    every layer at step-counter values 0..7, and without a step counter."""
    Fn = _fn()
    from wav2vec2forbrain_amd.train import step_graph
    g = torch.Generator().manual_seed(n)
    seeds = [int(s) for s in torch.randint(0, 2 ** 62, (n,), generator=g)]
    arr = (ctypes.c_uint64 * n)(*seeds)
    flags = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    epoch = torch.zeros(1, dtype=torch.int64, device="cuda")
    p = 0.5
    try:
        for e in [None] + list(range(8)):
            if e is not None:
                epoch.fill_(e)
                step_graph._install_epoch(epoch)
            _call("b2p_layerdrop_flags", P(flags), arr, n, p)
            torch.cuda.synchronize()
            got = flags.tolist()
            assert got[n] == -7                       # nothing written past the n flags
            assert got[:n] == [int(Fn.layerdrop_keep(p, s, e)) for s in seeds], e
    finally:
        step_graph._install_epoch(None)


# ------------------------------------------------------------------ layer level
P_LD = 0.5
REPLAYS = 8
LAYERS = 3


def _ld_seed():
    """A LD_SEEDS reseed value under which, over step-counter values 1..REPLAYS, every layer is both kept
    and skipped at least once (found with the host draw; the test asserts it on the real replays)."""
    Fn = _fn()
    for r in range(1000):
        Fn.LD_SEEDS.reseed(r)
        seeds = [Fn.LD_SEEDS.next() for _ in range(LAYERS)]
        pats = [[Fn.layerdrop_keep(P_LD, s, e) for e in range(1, REPLAYS + 1)] for s in seeds]
        if all(any(p) and not all(p) for p in pats):
            return r
    raise AssertionError("no seed found")


def _run_encoder(fuse, f16, mode="bf16"):
    """REPLAYS replays of one captured step of a 3-layer post-LN encoder (D 128, 2 heads of 64, T' 40,
    B 2: the fused bf16 attention path; mode fp32: the fp32 post-LN layer): per replay the loss, the
    output, the input gradient and every parameter gradient; plus the keep pattern per replay and the
    LayerDrop launches the capture issued."""
    Fn = _fn()
    from wav2vec2forbrain_amd import _lib
    from wav2vec2forbrain_amd.model import w2v_config
    from wav2vec2forbrain_amd.model.w2v_custom_feat_extractor import Wav2Vec2Encoder
    from wav2vec2forbrain_amd.train.step_graph import StepGraph
    assert Fn.attn16_ok(40, 64)
    r = _ld_seed()
    torch.manual_seed(11)
    Fn.SEEDS.reseed(77)
    Fn.LD_SEEDS.reseed(r)
    cfg = w2v_config.W2VConfig(hidden_size=128, num_hidden_layers=LAYERS, num_attention_heads=2, intermediate_size=256,
                               num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, layerdrop=P_LD)
    enc = Wav2Vec2Encoder(cfg).cuda()
    enc.train()
    x = torch.randn(2, 40, 128, device="cuda", requires_grad=True)
    w = torch.randn(2, 40, 128, device="cuda")
    box = {}

    def step():
        x.grad = None
        for p in enc.parameters():
            p.grad = None
        out = enc(x)
        loss = (out * w).sum()
        loss.backward()
        box["out"] = out.detach()
        return loss.detach()

    calls = []
    orig = _lib.call

    def spy(name, *a):
        if name.startswith("b2p_layerdrop_"):
            calls.append(name)
        return orig(name, *a)

    Fn._LD_FUSE = fuse
    Fn.LAYERDROP_LOG = []
    _lib.call = spy
    recs, pats = [], []
    try:
        with Fn.precision(mode), Fn.forward_f16(f16):
            sg = StepGraph(step, None, warmup=0, warm_replays=0)
            sg.capture()
            seeds = list(Fn.LAYERDROP_LOG)
            for _ in range(REPLAYS):
                loss = sg.replay()
                torch.cuda.synchronize()
                ep = int(sg.epoch.item())
                pats.append(tuple(Fn.layerdrop_keep(P_LD, s, ep) for s in seeds))
                rec = {"loss": loss.clone(), "out": box["out"].clone(), "x.grad": x.grad.clone()}
                rec.update({n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None})
                recs.append(rec)
            sg.release()
    finally:
        _lib.call = orig
        Fn._LD_FUSE = True
        Fn.LAYERDROP_LOG = None
    torch.cuda.synchronize()
    return recs, pats, calls, seeds


@pytest.mark.parametrize("mode,f16", [("bf16", False), ("bf16", True), ("fp32", False)])
def test_fused_layerdrop_encoder_bitwise(mode, f16):
    """The converted layer forms (_EncoderLayer16 with forward_f16 off and on, the fp32 _EncoderLayer) with the
    fold on and off: the same draws, no select / route launch and one flag launch with it on, and per
    replay bitwise-equal loss, output, input gradient and parameter gradients."""
    on, pats_on, calls_on, seeds_on = _run_encoder(True, f16, mode)
    off, pats_off, calls_off, seeds_off = _run_encoder(False, f16, mode)
    assert seeds_on == seeds_off and pats_on == pats_off and len(seeds_on) == LAYERS
    for k in range(LAYERS):   # not vacuous: every layer both kept and skipped within the replays
        col = [p[k] for p in pats_on]
        assert any(col) and not all(col), (k, pats_on)
    # the fold launches one flag kernel and nothing else; the switch restores the three launches per layer
    assert calls_on == ["b2p_layerdrop_flags"], calls_on
    assert sorted(calls_off) == sorted(["b2p_layerdrop_flag", "b2p_layerdrop_select_h", "b2p_layerdrop_route"] * LAYERS)
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.keys() == b.keys()
        for n in a:
            assert _same(a[n], b[n]), (i, n, pats_on[i])
        assert bool(torch.isfinite(a["loss"])) and bool(torch.isfinite(a["x.grad"]).all())
