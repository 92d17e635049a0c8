"""Times the fused bf16 attention kernels at the bench shape (B=32, T=249, 12 heads x 64).
usage: python tools/attn_bench.py [--parts] [B] [T] [nh]
--parts: also the backward that leaves the Q/K/V bias gradients as per-tile partial sums and writes no fp32
dqkv image (b2p_attn16_bwd_parts), beside the backward with the image plus the column sum that read it.
usage: python tools/attn_bench.py --fp32 [B T nh]
the fp32 / bf16x3 modes' attention core: fused exact-fp32 kernels (both shape classes) against the unfused GEMMs +
softmax, at the given shape or at the default list."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wav2vec2forbrain_amd import functional as Fn


def timeit(f, n=10):
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


FP32_SHAPES = ((32, 249, 12), (8, 249, 16),                   # the 256 class: base, Conformer-large fine-tune
               (8, 313, 16), (8, 512, 16), (32, 313, 12))     # the long class: 1,280-bin windows, the limit, base


def fp32_ab(shapes=FP32_SHAPES):
    """--fp32: the fp32 / bf16x3 modes' attention core, fused (csrc/attn32.hip) against unfused (6 batched GEMMs +
    2 softmax kernels, functional.fused_attn32(False)), forward and backward, at the base and the Conformer-large
    fine-tune shapes of both shape classes, in both modes; and the bytes each form keeps for the backward."""
    dh = 64
    Fn.ATTN32_MODES = (1, 3)   # the kernels against the fp32 mode's unfused form too (its default stays unfused)
    for B, T, nh in shapes:
        qkv = torch.randn(B * T, 3 * nh * dh, device="cuda") * 0.5
        dO = torch.randn(B * T, nh * dh, device="cuda")
        for mode in ("fp32", "bf16x3"):
            for p in (0.0, 0.1):
                res = {}
                for fused in (True, False):
                    with Fn.precision(mode), Fn.fused_attn32(fused):
                        fwd = lambda: Fn._attn_core_fwd(qkv, B, T, nh, dh, p, 5)
                        P, Pd, _ = fwd()
                        assert (P.dim() == 3) == fused
                        tf = timeit(fwd)
                        tb = timeit(lambda: Fn._attn_core_bwd(qkv, P, Pd, dO, B, T, nh, dh, p, 5))
                    kept = sum(t.numel() * t.element_size() for t in (P, Pd) if t is not None)
                    res[fused] = (tf, tb, kept)
                    del P, Pd
                (ff, fb, fk), (uf, ub, uk) = res[True], res[False]
                fl = 4.0 * B * nh * T * T * dh
                print(f"attn32[{mode}] B={B} T={T} nh={nh} p={p}: fwd fused {ff:.1f} us ({fl / ff / 1e6:.0f} TFLOP/s) "
                      f"unfused {uf:.1f} us; bwd fused {fb:.1f} us ({3.5 * fl / fb / 1e6:.0f} TFLOP/s) unfused {ub:.1f} us; "
                      f"fwd+bwd {ff + fb:.1f} vs {uf + ub:.1f} us ({(uf + ub) / (ff + fb):.2f}x); kept for the backward "
                      f"{fk / 1e6:.2f} MB vs {uk / 1e6:.2f} MB", flush=True)


if "--fp32" in sys.argv:
    shape = [int(a) for a in sys.argv[1:] if a != "--fp32"]
    if shape and len(shape) != 3:
        sys.exit("usage: python tools/attn_bench.py --fp32 [B T nh]")
    fp32_ab((tuple(shape),) if shape else FP32_SHAPES)
    sys.exit(0)
PARTS = "--parts" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--parts"]
B = int(argv[0]) if len(argv) > 0 else 32
T = int(argv[1]) if len(argv) > 1 else 249
nh = int(argv[2]) if len(argv) > 2 else 12
dh = 64
q = torch.randn(B * T, 3 * nh * dh, device="cuda") * 0.5
dO = torch.randn(B * T, nh * dh, device="cuda").to(torch.bfloat16)
fl = 4.0 * B * nh * T * T * dh
for kind in ("f16", "bf16"):
    for p in (0.0, 0.1):
        if kind == "f16":
            q16 = q.to(torch.float16)
            fwd = lambda: Fn._attn16_fwd_f16(q16, B, T, nh, dh, p, 5)
            _, _, lse2, mask = fwd()
        else:
            q16 = q.to(torch.bfloat16)
            fwd = lambda: Fn._attn16_fwd(q16, B, T, nh, dh, p, 5, want_mask=True)
            _, lse2, mask = fwd()
        tf = timeit(fwd)
        tb = timeit(lambda: Fn._attn16_bwd(q16, dO, lse2, B, T, nh, dh, p, 5, mask=mask))
        print(f"attn16[{kind}] B={B} T={T} nh={nh} p={p}: fwd {tf:.1f} us ({fl / tf / 1e6:.0f} TFLOP/s), "
              f"bwd {tb:.1f} us ({2.5 * fl / tb / 1e6:.0f} TFLOP/s)", flush=True)
        if PARTS:
            D = nh * dh
            db = torch.empty(3 * D, device="cuda")

            def old():   # fp32 image + the column sum that was its only reader
                d32, _ = Fn._attn16_bwd(q16, dO, lse2, B, T, nh, dh, p, 5, mask=mask)
                Fn.colsum(d32, B * T, 3 * D, db)

            def new():   # no image: per-tile partials, finished by one column sum per plane
                _, _, bp = Fn._attn16_bwd(q16, dO, lse2, B, T, nh, dh, p, 5, want32=False, mask=mask, bias_parts=True)
                for g in bp:
                    g.materialize()

            to, tn = timeit(old), timeit(new)
            tk = timeit(lambda: Fn._attn16_bwd(q16, dO, lse2, B, T, nh, dh, p, 5, want32=False, mask=mask,
                                               bias_parts=True))
            print(f"    bias gradients: fp32 image + colsum {to:.1f} us; partials, no image {tk:.1f} us "
                  f"(+ 3 partial sums: {tn:.1f} us)", flush=True)
# the bf16 mode's forward with the keep bits drawn ahead (functional.attn_keep_plan: b2p_attn16_keep_masks
# + b2p_attn16_fwd_f16_keep, DM 3), and the draw itself for one layer
import ctypes
q16 = q.to(torch.float16)
masks = torch.empty(1, B, nh, T, 8, device="cuda", dtype=torch.int32)
seeds = (ctypes.c_uint64 * 1)(5)
draw = lambda: Fn._lib.call("b2p_attn16_keep_masks", masks.data_ptr(), ctypes.addressof(seeds), 1, B, T, nh, 0.1, Fn._st())
draw()
Oh = torch.empty(B * T, nh * dh, device="cuda", dtype=torch.float16)
Ob = torch.empty(B * T, nh * dh, device="cuda", dtype=torch.bfloat16)
lse2 = torch.empty(B, nh, T, device="cuda")
fk = lambda: Fn._lib.call("b2p_attn16_fwd_f16_keep", q16.data_ptr(), Oh.data_ptr(), Ob.data_ptr(), lse2.data_ptr(), B, T,
                          nh, dh, float(dh ** -0.5), 0.1, masks[0].data_ptr(), Fn._st())
tf, td = timeit(fk), timeit(draw)
print(f"attn16[f16, keep bits read] B={B} T={T} nh={nh} p=0.1: fwd {tf:.1f} us ({fl / tf / 1e6:.0f} TFLOP/s); "
      f"keep-mask draw {td:.1f} us per layer", flush=True)
