"""The fused attention backward with bias partials and no fp32 image (b2p_attn16_bwd_parts) against the
existing entry points (b2p_attn16_bwd / b2p_attn16_bwd_f16, tied to the oracle by tests/test_kernels_gpu.py).

Per column of dqkv, with x the fp32 image the existing entry point writes for the same inputs, summed over
its n = B * T rows in float64:

    |sum(partial rows) - sum64(x)| <= n * 2^-24 * sum|x|

the worst-case bound of any fp32 summation order of n terms (each of at most n - 1 additions rounds by
2^-24 relative to a partial sum that sum|x| bounds), so no order the kernels may choose needs a tuned
tolerance. dqkv16 and delta are bitwise the existing entry point's; a closed LayerDrop gate gives exactly
zero sums; two launches into a NaN-filled and a zero-filled buffer give bitwise-identical partials (every
element written, nothing accumulated into).

B = 2, two heads of 64. T: 17 (waves and tiles beyond T), 130 (a second, almost empty 128-block: the
dK/dV early exit), 249 (the workload's T' and the T1 form), 256 (full tiles), 300 (the 512-row kernels,
dropout none / hashed only). Both operand precisions, both dK/dV kernels, the gate open and closed."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, NH, DH = 2, 2, 64
D = NH * DH
SEED = 4242
P_DROP = 0.1


def _forward(Fn, T, half, mode):
    """qkv16, dO16, lse2, the keep bits (stored mode only) and the dropout p of one forward."""
    g = torch.Generator().manual_seed(1000 * T + 10 * int(half) + len(mode))
    qkv = (torch.randn(B * T, 3 * D, generator=g) * 0.7).cuda()
    dO = torch.randn(B * T, D, generator=g).to(torch.bfloat16).cuda()
    p = 0.0 if mode == "none" else P_DROP
    if half:
        q16 = qkv.to(torch.float16)
        _, _, lse2, mask = Fn._attn16_fwd_f16(q16, B, T, NH, DH, p, SEED)
    else:
        q16 = qkv.to(torch.bfloat16)
        out = Fn._attn16_fwd(q16, B, T, NH, DH, p, SEED, want_mask=(mode == "stored"))
        lse2, mask = out[1], (out[2] if len(out) > 2 else None)
    if mode == "stored":
        assert mask is not None
    else:
        mask = None   # hashed: the backward re-draws the bits from the seed
    return q16, dO, lse2, mask, p


def _old(Fn, q16, dO, lse2, mask, p, T):
    d32 = torch.full((B * T, 3 * D), float("nan"), device="cuda")
    d16 = torch.empty(B * T, 3 * D, device="cuda", dtype=torch.bfloat16)
    delta = torch.zeros(B, NH, T, device="cuda")
    fn = "b2p_attn16_bwd_f16" if q16.dtype == torch.float16 else "b2p_attn16_bwd"
    Fn._lib.call(fn, Fn._p(q16), Fn._p(dO), Fn._p(lse2), Fn._p(delta), Fn._p(d32), Fn._p(d16), B, T, NH, DH,
                 float(DH ** -0.5), float(p), SEED, None if mask is None else mask.data_ptr(), Fn._st())
    return d32, d16, delta


def _new(Fn, q16, dO, lse2, mask, p, T, fill):
    rows = int(Fn._lib.load().b2p_attn16_bwd_bias_parts_rows(B, T, NH))
    assert rows > 0
    parts = torch.full((3, rows, D), fill, device="cuda")
    d16 = torch.empty(B * T, 3 * D, device="cuda", dtype=torch.bfloat16)
    delta = torch.zeros(B, NH, T, device="cuda")
    Fn._lib.call("b2p_attn16_bwd_parts", int(q16.dtype == torch.float16), Fn._p(q16), Fn._p(dO), Fn._p(lse2),
                 Fn._p(delta), None, Fn._p(d16), Fn._p(parts), B, T, NH, DH, float(DH ** -0.5), float(p), SEED,
                 None if mask is None else mask.data_ptr(), Fn._st())
    return parts, d16, delta


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("half", [True, False], ids=["f16", "bf16"])
@pytest.mark.parametrize("T", [17, 130, 249, 256, 300])
def test_bias_partials_against_fp32_image(T, half):
    from wav2vec2forbrain_amd import functional as Fn
    lib = Fn._lib.load()
    n = B * T
    modes = ("none", "hashed", "stored") if T <= 256 else ("none", "hashed")
    closed = torch.zeros(1, dtype=torch.int32, device="cuda")
    opened = torch.ones(1, dtype=torch.int32, device="cuda")
    try:
        for mode in modes:
            q16, dO, lse2, mask, p = _forward(Fn, T, half, mode)
            per_variant = []
            for variant in (1, 0):
                Fn._lib.check(lib.b2p_attn16_dkv_variant(variant), "dkv_variant")
                tag = (T, half, mode, variant)
                for gate in (None, opened, closed):
                    with Fn._gated(gate):
                        d32, d16, delta = _old(Fn, q16, dO, lse2, mask, p, T)
                        parts, n16, ndelta = _new(Fn, q16, dO, lse2, mask, p, T, float("nan"))
                        parts0, _, _ = _new(Fn, q16, dO, lse2, mask, p, T, 0.0)
                    torch.cuda.synchronize()
                    assert _bits(n16, d16), tag
                    assert _bits(parts, parts0), tag          # full coverage, nothing accumulated into
                    assert bool(torch.isfinite(parts).all()), tag
                    got = parts.double().sum(1).reshape(3 * D)
                    if gate is closed:
                        assert float(parts.abs().max()) == 0.0, tag
                        assert float(d32.abs().max()) == 0.0 and float(d16.float().abs().max()) == 0.0, tag
                        continue
                    assert _bits(ndelta, delta), tag
                    x = d32.double()
                    ref, mag = x.sum(0), x.abs().sum(0)
                    err = (got - ref).abs()
                    bound = n * 2.0 ** -24 * mag
                    worst = float((err / bound.clamp(min=1e-300)).max())
                    print(f"T={T} half={half} mode={mode} variant={variant} gate={'open' if gate is not None else 'none'}: "
                          f"max err/bound {worst:.3e}")
                    assert bool((err <= bound).all()), (tag, worst)
                    assert float(mag.min()) > 0, tag         # every column carries signal
                    if gate is None:
                        per_variant.append(parts)
            assert _bits(per_variant[0], per_variant[1]), (T, half, mode)   # both dK/dV kernels: the same partials
    finally:
        Fn._lib.check(lib.b2p_attn16_dkv_variant(1), "dkv_variant")


def test_python_wrapper_returns_three_planes():
    """_attn16_bwd(bias_parts=True): three ColsumParts whose sums are the planes' column sums; with
    want32=False no fp32 image is returned, the default call still returns it."""
    from wav2vec2forbrain_amd import functional as Fn
    T = 40
    q16, dO, lse2, mask, p = _forward(Fn, T, True, "stored")
    d32, d16 = Fn._attn16_bwd(q16, dO, lse2, B, T, NH, DH, p, SEED, mask=mask)
    none32, n16, bp = Fn._attn16_bwd(q16, dO, lse2, B, T, NH, DH, p, SEED, want32=False, mask=mask, bias_parts=True)
    torch.cuda.synchronize()
    assert none32 is None and d32 is not None and _bits(n16, d16)
    assert len(bp) == 3 and all(isinstance(g, Fn.ColsumParts) for g in bp)
    x = d32.double()
    for q, g in enumerate(bp):
        got = g.materialize().double()
        ref, mag = x[:, q * D:(q + 1) * D].sum(0), x[:, q * D:(q + 1) * D].abs().sum(0)
        # the partial rows and their fp32 sum together are still one fp32 summation order of the n values
        assert bool(((got - ref).abs() <= B * T * 2.0 ** -24 * mag).all())
