"""Step-level A/B of the multi-CU persistent GRU recurrence at hidden size 1024 (csrc/grumc.hip): replayed
Trainer.train_step of workloads.bench_config("base") with gru_hidden=1024, gru_layers=3 (the reference sweeps'
largest brain encoder under the bench's base w2v model, bf16 mode), with functional._GRUMC off (the per-time-step
kernels) and on, alternating in one process, two runs each. Per run: ms per step (warm-up steps eager, one
capture, then timed replays; losses read after the timed region), the last loss, and
torch.cuda.max_memory_allocated() since the run began.
--full: the full fine-tune instead (the w2v encoder optimised too, so the Trainer switches to the bf16x3 mode): the
A/B is then the policy's forms, the default ('gru32w': the persistent exact-fp32 recurrence, csrc/gru32.hip) against
'grurec1' in its place (the 16-bit recurrence of csrc/grumc.hip inside the bf16x3 mode).
usage: python tools/gru1024_step_ab.py [--full] [--bs 32] [--seq 1024] [--steps 10] [--warmup 3] [--hidden 1024]
       [--layers 3]"""
import argparse
import gc
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wav2vec2forbrain_amd import functional as Fn
from wav2vec2forbrain_amd.train.train_loop import Trainer
from wav2vec2forbrain_amd.workloads import SyntheticStepExperiment, bench_config, build_model, device_batch


def run(cfg, steps, warmup, mc, forms=None):
    """mc: functional._GRUMC for the run; forms: None, or the full fine-tune's bf16x3 policy forms."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    old, Fn._GRUMC[0] = Fn._GRUMC[0], mc
    old_forms = Fn.X3_POLICY_FORMS
    try:
        if forms is not None:
            Fn.X3_POLICY_FORMS = frozenset(forms)
        model = build_model(cfg, device="cuda", train_dropouts=True)
        model.train()
        for m in model.modules():
            if hasattr(m, "sync_metrics"):
                m.sync_metrics = False      # no host sync per step: the losses are read after the timed region
        trainer = Trainer(SyntheticStepExperiment(model, lr=1e-3, **({} if forms is None else
                                                                  {"unfreeze": "brain_encoder+w2v"})))
        trainer.capture_after = warmup
        batch = device_batch(cfg, "cuda")
        with trainer.precision_context():
            rec = Fn._gru_recurrence(cfg["gru_hidden"])
        for _ in range(warmup + (1 if trainer.use_graphs else 0)):
            trainer.train_step(batch)
        torch.cuda.synchronize()
        losses = torch.zeros(steps, device="cuda")
        g0 = trainer.graph_steps
        t0 = time.perf_counter()
        for i in range(steps):
            losses[i] = trainer.train_step(batch).loss.detach().reshape(())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        replayed = trainer.graph_steps - g0
        Fn.check_gru_status()
        mode = "hip-graph replay" if replayed == steps else "eager" if replayed == 0 else f"mixed ({replayed}/{steps})"
        res = (dt / steps * 1e3, mode, float(losses[-1]), torch.cuda.max_memory_allocated() / 2 ** 20, rec)
        trainer.release_graphs()
        Fn.set_deferred_wgrad([])
        del trainer, model, batch
    finally:
        Fn._GRUMC[0] = old
        Fn.X3_POLICY_FORMS = old_forms
    gc.collect()
    torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--full", action="store_true")
    a = ap.parse_args()
    cfg = dict(bench_config("base", a.bs, a.seq), gru_hidden=a.hidden, gru_layers=a.layers)
    print(f"base w2v, GRU H={a.hidden} x {a.layers} layers, bs {a.bs}, L {a.seq}, {a.steps} timed steps after {a.warmup} "
          "warm-up", flush=True)
    gemm_forms = Fn.X3_POLICY_FORMS - {"gru32w", "grurec1"}
    # (label, _GRUMC, policy forms)
    arms = ([("gru32w ", True, gemm_forms | {"gru32w"}), ("grurec1", True, gemm_forms | {"grurec1"})] if a.full else
            [("mc off", False, None), ("mc on ", True, None)])
    if a.full:
        print("full fine-tune (bf16x3 policy); no reference trajectory exists at this size: times and memory only",
              flush=True)
    for r in range(2):
        for label, mc, forms in arms:
            try:
                ms, mode, loss, peak, rec = run(cfg, a.steps, a.warmup, mc, forms)
            except RuntimeError as e:   # the per-step backward (csrc/gru.hip) has no H = 1024
                Fn.set_deferred_wgrad([])
                gc.collect()
                torch.cuda.empty_cache()
                print(f"run {r} {label}: no step ({e})", flush=True)
                continue
            print(f"run {r} {label} ({rec}): {ms:.3f} ms/step ({mode}), last loss {loss:.6f}, "
                  f"peak {peak:.0f} MiB", flush=True)
    print(f"gru status word {Fn.gru_status_value()}", flush=True)
