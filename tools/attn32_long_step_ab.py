"""Step-level A/B of the bf16x3 mode's fused exact-fp32 attention on the Conformer-large fine-tune workload
(the conformer_large_ft_bs8 architecture, B = 8, unfreeze brain_encoder+w2v) at a window length whose T' lies
in the long class (default 1,280 bins: T' = 313): bench.py's own timed_run with functional.fused_attn32 off (the
unfused batched GEMMs + softmax) and on, alternating in one process.
usage: python tools/attn32_long_step_ab.py [--seq 1280] [--steps 10] [--warmup 3] [--runs 2]
Prints ms per replayed step, torch.cuda.max_memory_allocated() since the run began, and the batched attention
GEMMs the eager warm-up steps issued (0 when the fused kernels ran)."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from wav2vec2forbrain_amd import build_lib, functional as Fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    build_lib.ensure_built()
    torch.manual_seed(1234)
    ns = argparse.Namespace(steps=a.steps, warmup=a.warmup, bs=bench.FT["bs"], seq=a.seq, evaluator=False,
                            no_roofline=True)
    for run in range(a.runs):
        for fused in (False, True):
            bench.free_device()
            torch.cuda.reset_peak_memory_stats()
            Fn.GEMM_LOG = []
            try:
                with Fn.fused_attn32(fused):
                    r = bench.timed_run("conformer_ft", ns, 1, 0, "cuda:0", True)
                cfg = r["cfg"]
                batched = [e for e in Fn.GEMM_LOG if e["nz"] == cfg["B"] * cfg["heads"]]
            finally:
                Fn.GEMM_LOG = None
            Ts = sorted({e["M"] for e in batched})
            print(f"conformer_large_ft L={a.seq} run {run} fused_attn32 {'on ' if fused else 'off'}: "
                  f"{r['dt'] / r['steps'] * 1e3:.3f} ms/step ({r['step_mode']}, {r['precision']}), last loss "
                  f"{r['losses'][-1]:.6f}, peak {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB, batched attention "
                  f"GEMMs in the eager steps {len(batched)} (T' {Ts})", flush=True)


if __name__ == "__main__":
    main()
