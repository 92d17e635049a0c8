"""Measured error and time of the activation-table kernels (b2p_act_fwd / b2p_act_bwd) on the device.

Errors: per id, the maximum of |kernel - truth| / max(1, |truth|) over the kernel tests' points
(tests/act_cases.grid: 1,024 points on [-12, 12] and +-30 .. +-1e30), value and derivative, against
float64 torch; beside it the same figure for torch's own fp32 CPU kernels on the same points.
Times: device events around 200 launches at the Conformer-large fc shape (7,968 x 256 fp32), the
operands rotating through 16 buffer sets (~390 MB) so the 256 MB last-level cache does not hold them;
and the fc layer's forward as the fused gelu epilogue runs it against GEMM + b2p_act_fwd.

usage: python tools/act_errors.py [out.txt]
"""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import act_cases as AC  # noqa: E402


def _ratio(got, want):
    got, want = got.detach().double().cpu(), want.double()
    ok = want.abs() <= torch.finfo(torch.float32).max
    return float(((got[ok] - want[ok]).abs() / want[ok].abs().clamp_min(1.0)).max())


def _timed(fn, sets, iters=200, warm=20):
    for i in range(warm):
        fn(sets[i % len(sets)])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


def main():
    from wav2vec2forbrain_amd import build_lib
    build_lib.ensure_built()
    from wav2vec2forbrain_amd import functional as Fn
    out = []
    x = AC.grid()
    xd = x.cuda()
    one = torch.ones_like(xd)
    out.append(f"max |result - float64 truth| / max(1, |truth|) in units of 2^-24, {x.numel()} points; "
               f"the kernel tests' bound is 16")
    out.append(f"{'id':>2} {'function':<11} {'value: kernel':>14} {'torch fp32 CPU':>15} {'derivative: kernel':>19} "
               f"{'torch fp32 CPU':>15}")
    for act in range(AC.ID_LAST + 1):
        name = AC.ID_NAME[act]
        v, g = AC.truth(name, x)
        kv = _ratio(Fn.act_fwd(xd, act), v)
        kg = _ratio(Fn._act_bwd(one, xd, act), g)
        xc = x.clone().requires_grad_(True)
        yc = AC.FN[name](xc)
        (gc,) = torch.autograd.grad(yc.sum(), xc) if yc.requires_grad else (torch.zeros_like(xc),)
        nan = int(torch.isnan(yc).sum() + torch.isnan(gc).sum())
        fin = ~(torch.isnan(yc) | torch.isnan(gc))
        u = 2.0 ** 24
        out.append(f"{act:>2} {name:<11} {kv * u:>14.2f} {_ratio(yc[fin], v[fin]) * u:>15.2f} {kg * u:>19.2f} "
                   f"{_ratio(gc[fin], g[fin]) * u:>15.2f}" + (f"   (torch fp32: {nan} NaN left out)" if nan else ""))
    M, N, K = 7968, 256, 1024
    n = M * N
    sets = [tuple(torch.randn(n, device="cuda") for _ in range(3)) for _ in range(16)]
    out.append("")
    out.append(f"time per launch, {M} x {N} fp32 ({n * 4 / 1e6:.1f} MB per tensor), us (GB/s of the 8 / 12 bytes per "
               f"element moved)")
    for act in (0, 1, 4, 5, 7, 8, 9, 13):
        tf = _timed(lambda s: Fn.act_fwd(s[0], act, s[2]), sets)
        tb = _timed(lambda s: Fn._act_bwd(s[1], s[0], act, s[2]), sets)
        out.append(f"{AC.ID_NAME[act]:<11} b2p_act_fwd {tf:7.2f} ({8 * n / tf / 1e3:6.0f})   b2p_act_bwd {tb:7.2f} "
                   f"({12 * n / tb / 1e3:6.0f})")
    out.append("")
    out.append(f"the fc layer's forward, x[{M}, {K}] @ W[{N}, {K}]^T + b, us per call (the GEMM kernels are the "
               f"parent's, unchanged)")
    xs = [(torch.randn(M, K, device="cuda"), torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda"))
          for _ in range(8)]
    W = torch.randn(N, K, device="cuda") / 32
    b = torch.randn(N, device="cuda")
    for mode in ("bf16", "fp32"):
        with Fn.precision(mode):
            fused = _timed(lambda s: Fn.mm_nt(s[0], W, s[1], bias=b, act=Fn.ACT["gelu"], pre_out=s[2]), xs)
            plain = _timed(lambda s: Fn.mm_nt(s[0], W, s[2], bias=b), xs)
            split = _timed(lambda s: (Fn.mm_nt(s[0], W, s[2], bias=b), Fn.act_fwd(s[2], Fn.ACT["relu"], s[1])), xs)
        out.append(f"{mode}: GEMM with the fused gelu epilogue (pre-activation kept) {fused:.2f}; GEMM with bias alone "
                   f"{plain:.2f}; GEMM with bias + b2p_act_fwd(relu) {split:.2f}")
    text = "\n".join(out) + "\n"
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
