"""The rule of tests/attn16_cases.py tested on the host: the per-element bound that tests/test_attn16_edges_gpu.py
holds the fused 16-bit attention (csrc/attn16.hip) to is applied to a float64 emulation of the kernels that rounds
exactly where they round, and to the same emulation with a defect built in. No device is needed and no kernel is
ever made wrong.

The emulation (emulate) follows the kernels' data flow in float64 and rounds (through fp32, as the kernels do) at
their 16-bit rounding points only:
  forward   P_d = e / sum * keep / (1 - p) -> operand type (bf16, fp16 in the fp16 mode); O -> operand type; the fp16
            mode's bf16 copy Ob from the unrounded O; lse2 = zmax + log2(sum)
  backward  P = exp2(z - lse2); fp16 mode: V -> bf16 for dP, Q -> bf16 for dK, K -> bf16 for dQ in the 512-key class;
            delta = sum_key P dP keep / (1 - p); dV from P_d -> bf16; dK from dS -> bf16; dQ from dS -> bf16, or in the
            fp16 mode at T' <= 256 from the row scaled by the power of two that puts its largest |dS| in [1, 2) -> fp16;
            the bf16 image dqkv16 of the gradients
Its fp32 arithmetic is exact, so it exercises the 16-bit terms of the bound.

(a) The clean emulation lies within the bound at every element of every output, at every T' of the GPU test, in both
    operand types and at both p, on the GPU test's own (spiked) inputs.
(b) Each defect, on the same inputs without the spikes (a spike would make the defects easy), puts at least one
    element of O or of the fp32 gradient image outside the bound at every T' >= 2; lse2 and delta, whose bounds hold
    fp32 terms only and so catch any change of the scores at once, are left out of this verdict on purpose:
      drop    the last key left out and the row renormalised, for the queries of the last 16-row tile only
      keep    the keep bit of key T' - 1 inverted (at p = 0: the key dropped as if its bit were clear)
      scale   the scores of the last tile's queries multiplied by 1.05
Figures (worst |err| / bound over every T', p and output): clean 0.916 (dqkv) and 0.824 (Ob). Smallest excess of a
defect on O or dqkv: drop 3.7 (bf16, T' = 497) and 16 (fp16); keep 52; scale 1.46 (bf16, T' = 385) and 7.6 (fp16). A
margin of 2 on the bound would let the scaled scores through in the bf16 mode: there is none.
"""
import pytest
import torch

from tests import attn16_cases as C

B, NH, D, SCALE = C.B, C.NH, C.D, C.SCALE


def r16(x, dtype):
    return x.to(torch.float32).to(dtype).double()


def bf(x):
    return r16(x, torch.bfloat16)


def emulate(qkv16, dO16, T, half, keep, p, defect=None):
    x = qkv16.double()
    q, k, v = (C.heads(x[:, i * D:(i + 1) * D], T) for i in range(3))
    dOh = C.heads(dO16.double(), T)
    op = torch.float16 if half else torch.bfloat16
    t = lambda a: a.transpose(-1, -2)
    last = slice(16 * ((T - 1) // 16), T)        # the queries of the last 16-row tile
    ks = torch.ones(B, NH, T, T, dtype=torch.float64) if keep is None else keep.double() / (1.0 - p)
    z = q @ t(k) * SCALE * C.LOG2E
    valid = torch.ones(T, T, dtype=torch.bool)
    if defect == "drop":
        valid[last, T - 1] = False
    elif defect == "keep":
        ks = ks.clone()
        ks[..., T - 1] = torch.where(ks[..., T - 1] > 0, 0.0, 1.0 / (1.0 - p))
    elif defect == "scale":
        z = z.clone()
        z[:, :, last] *= 1.05
    z = z.masked_fill(~valid, float("-inf"))
    zmax = z.amax(-1, keepdim=True)
    e = torch.exp2(z - zmax)
    s = e.sum(-1, keepdim=True)
    lse2 = (zmax + torch.log2(s))[..., 0]
    O32 = r16(e / s * ks, op) @ v
    out = {"O": C.rows(r16(O32, op), T), "lse2": lse2}
    if half:
        out["Ob"] = C.rows(bf(O32), T)
    P = torch.exp2(z - lse2[..., None])
    vb, qb, kb = (bf(v), bf(q), bf(k)) if half else (v, q, k)
    PD = (dOh @ t(vb)) * ks
    delta = (P * PD).sum(-1)
    dS = P * (PD - delta[..., None])
    dV = t(bf(P * ks)) @ dOh
    dK = t(bf(dS)) @ qb * SCALE
    if half and T <= 256:
        mx = dS.abs().amax(-1, keepdim=True)
        pw = torch.exp2(torch.floor(torch.log2(torch.where(mx > 0, mx, torch.ones_like(mx)))))
        dQ = (r16(dS / pw, torch.float16) @ k) * pw * SCALE
    else:
        dQ = bf(dS) @ kb * SCALE
    dqkv = torch.cat([C.rows(dQ, T), C.rows(dK, T), C.rows(dV, T)], 1)
    out.update(delta=delta, dqkv=dqkv, dqkv16=bf(dqkv))
    return out


def _setup(T, half, p, spikes):
    qkv16, dO16 = C.operands(T, half, spikes)
    keep = C.keep_ref(T) if p > 0 else None
    r = C.ref64(qkv16, dO16, T, keep, p)
    return qkv16, dO16, keep, r, C.bounds(r, half)


MODES = [pytest.param(False, id="bf16"), pytest.param(True, id="fp16")]
PS = [pytest.param(0.0, id="p0"), pytest.param(C.P_DROP, id="p0.1")]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("half", MODES)
@pytest.mark.parametrize("T", C.T_ALL)
def test_clean_emulation_within_bound(T, half, p):
    qkv16, dO16, keep, r, bnd = _setup(T, half, p, True)
    ratios = C.worst_ratios(emulate(qkv16, dO16, T, half, keep, p), r, bnd)
    print(f"T'={T} {'fp16' if half else 'bf16'} p={p:.1f} clean: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("half", MODES)
@pytest.mark.parametrize("T", [T for T in C.T_ALL if T >= 2])
def test_defects_are_rejected(T, half, p):
    qkv16, dO16, keep, r, bnd = _setup(T, half, p, False)
    clean = C.worst_ratios(emulate(qkv16, dO16, T, half, keep, p), r, bnd)
    assert all(v <= 1.0 for v in clean.values()), clean
    missed = []
    for defect in ("drop", "keep", "scale"):
        ratios = C.worst_ratios(emulate(qkv16, dO16, T, half, keep, p, defect), r, bnd)
        print(f"T'={T} {'fp16' if half else 'bf16'} p={p:.1f} {defect}: " + " ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
        if not max(ratios["O"], ratios["dqkv"]) > 1.0:
            missed.append((defect, ratios))
    assert not missed, missed


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("T", C.T_EPOCH)
def test_clean_emulation_fp16_operands_that_are_no_bf16_numbers(T, p):
    """The inputs above are bf16 numbers even in the fp16 mode, so to_b16 in the backward is exact on them. Here qkv
    is rounded to fp16 directly: the residual terms of V, Q and K in the bound carry weight."""
    qkv16, dO16 = C.operands(T, True, via_bf16=False)
    assert float(C._res_bf16(qkv16.double()).max()) > 0
    keep = C.keep_ref(T) if p > 0 else None
    r = C.ref64(qkv16, dO16, T, keep, p)
    ratios = C.worst_ratios(emulate(qkv16, dO16, T, True, keep, p), r, C.bounds(r, True))
    print(f"T'={T} fp16-only qkv p={p:.1f} clean: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_seed_eff_and_mask_restatements():
    """seed_eff wraps at 64 bits and leaves the seed alone without a counter; the keep mask keeps about 1 - p of
    the elements, differs under another epoch, and is all ones at p = 0."""
    assert C.seed_eff(5) == 5 and C.seed_eff(5, 0) == 5
    assert C.seed_eff(2 ** 64 - 1, 1) == (2 ** 64 - 1 + 0x9E3779B97F4A7C15) % 2 ** 64
    assert C.seed_eff(C.SEED, C.EPOCH) == (C.SEED + 0x9E3779B97F4A7C15 * C.EPOCH) % 2 ** 64
    a, b = C.keep_ref(129), C.keep_ref(129, C.EPOCH)
    assert abs(float(a.double().mean()) - (1 - C.P_DROP)) < 0.01
    assert 0.1 < float((a != b).double().mean()) < 0.3          # two independent draws differ at 2 p (1 - p)
    assert C.keep_mask_ref(C.SEED, 0.0, 1, 1, 5).all()
