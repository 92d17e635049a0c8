"""Times one GRU layer's recurrence in the fp32-operand modes: the persistent exact-fp32 kernels
(csrc/gru32.hip: b2p_gru_fwd32 / b2p_gru_bwd32) against the per-time-step kernels (csrc/gru.hip: b2p_gru_fwd /
b2p_gru_bwd), forward and backward, both directions, through the C ABI (HIP-event time, 3 warm launches,
median of 11). Shapes: the Conformer-large fine-tune's (B 8, T' 249, H 512) and the bench batch (B 32, T' 249,
H 256 and 512). Also the largest difference of the two forms' outputs and the timeout flag. H = 1024 (P = 32
members; B 8 / 32 / 64 at T' 249 is the measured set) has no per-step backward: the forwards are compared and the
persistent backward is timed alone.
--mc: the same for the bf16 mode's multi-CU persistent kernels (csrc/grumc.hip: b2p_gru_fwd_mc / b2p_gru_bwd_mc;
H 256, 384, 512, 1024) against the per-time-step kernels.
usage: python tools/gru_bench.py [--mc] [B T H ...]"""
import math
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wav2vec2forbrain_amd import _lib


def timeit(f, warm=3, n=11):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


# persistent form -> (forward, backward, workspace) entry points
FORMS = {"gru32": ("b2p_gru_fwd32", "b2p_gru_bwd32", "b2p_gru32_workspace"),
         "mc": ("b2p_gru_fwd_mc", "b2p_gru_bwd_mc", "b2p_gru_mc_workspace")}


def bench(B, T, H, nd=2, new="gru32"):
    f_fwd, f_bwd, f_ws = FORMS[new]
    dev = "cuda"
    torch.manual_seed(1)
    gi = torch.randn(B, T, nd * 3 * H, device=dev)
    whh = torch.randn(nd, 3 * H, H, device=dev) / math.sqrt(H)
    bhh = torch.randn(nd, 3 * H, device=dev) * 0.1
    h0 = torch.randn(nd, B, H, device=dev)
    dout = torch.randn(B, T, nd * H, device=dev)
    st = _lib.stream_ptr()
    res = {}
    for form in (new, "per-step"):
        out = torch.empty(B, T, nd * H, device=dev)
        sv = torch.empty(B, T, nd, 4, H, device=dev)
        dgi = torch.empty(B, T, nd * 3 * H, device=dev)
        dgh = torch.empty_like(dgi)
        dh0 = torch.empty(nd, B, H, device=dev)
        if form == new:
            ws = torch.empty(int(getattr(_lib.load(), f_ws)(B, H, nd)), device=dev, dtype=torch.uint8)
            fwd = lambda: _lib.call(f_fwd, gi.data_ptr(), whh.data_ptr(), bhh.data_ptr(), h0.data_ptr(),
                                    out.data_ptr(), sv.data_ptr(), ws.data_ptr(), B, T, H, nd, st)
            bwd = lambda: _lib.call(f_bwd, dout.data_ptr(), whh.data_ptr(), out.data_ptr(), sv.data_ptr(),
                                    h0.data_ptr(), dgi.data_ptr(), dgh.data_ptr(), dh0.data_ptr(), ws.data_ptr(), B, T, H,
                                    nd, st)
        else:
            ws = None
            buf = torch.empty(nd, B, H, device=dev)
            fwd = lambda: _lib.call("b2p_gru_fwd", gi.data_ptr(), whh.data_ptr(), bhh.data_ptr(), h0.data_ptr(),
                                    out.data_ptr(), sv.data_ptr(), B, T, H, nd, st)
            bwd = lambda: _lib.call("b2p_gru_bwd", dout.data_ptr(), whh.data_ptr(), out.data_ptr(), sv.data_ptr(),
                                    h0.data_ptr(), dgi.data_ptr(), dgh.data_ptr(), dh0.data_ptr(), buf.data_ptr(), B, T, H,
                                    nd, st)
        tf = timeit(fwd)
        fail = 0 if ws is None else int(ws[:4].view(torch.int32).item())
        same = 0 if ws is None else int(ws[4:8].view(torch.int32).item())
        try:
            tb = timeit(bwd)
        except RuntimeError as e:   # the per-step backward stages 3H floats per row in LDS: no H = 1024
            if form == new:
                raise
            tb, no_bwd = None, str(e)
        fail |= 0 if ws is None else int(ws[:4].view(torch.int32).item())
        res[form] = (tf, tb, fail, same, [t.clone() for t in (out, dgi, dh0)])
    (nf, nb, fail, same, no), (sf, sb, _, _, so) = res[new], res["per-step"]
    if sb is None:   # forward only
        diff = float((no[0] - so[0]).abs().max())
        print(f"gru B={B} T={T} H={H} ndir={nd}: fwd {new} {nf[0]:.0f} us [{nf[1]:.0f}, {nf[2]:.0f}] ({nf[0] / T:.2f} us/step) "
              f"per-step {sf[0]:.0f} us [{sf[1]:.0f}, {sf[2]:.0f}] ({sf[0] / T:.2f} us/step, {sf[0] / nf[0]:.2f}x); bwd {new} "
              f"{nb[0]:.0f} us [{nb[1]:.0f}, {nb[2]:.0f}] ({nb[0] / T:.2f} us/step) per-step: none ({no_bwd}); "
              f"max |difference| (out) {diff:.2e}; timeout flag {fail}; recurrences on one XCD (last forward) {same}",
              flush=True)
        return
    diff = max(float((a - b).abs().max()) for a, b in zip(no, so))
    print(f"gru B={B} T={T} H={H} ndir={nd}: fwd {new} {nf[0]:.0f} us [{nf[1]:.0f}, {nf[2]:.0f}] ({nf[0] / T:.2f} us/step) "
          f"per-step {sf[0]:.0f} us [{sf[1]:.0f}, {sf[2]:.0f}] ({sf[0] / T:.2f} us/step); bwd {new} {nb[0]:.0f} us "
          f"[{nb[1]:.0f}, {nb[2]:.0f}] ({nb[0] / T:.2f} us/step) per-step {sb[0]:.0f} us [{sb[1]:.0f}, {sb[2]:.0f}] "
          f"({sb[0] / T:.2f} us/step); fwd+bwd {(nf[0] + nb[0]) / 1e3:.2f} vs {(sf[0] + sb[0]) / 1e3:.2f} ms "
          f"({(sf[0] + sb[0]) / (nf[0] + nb[0]):.2f}x); max |difference| {diff:.2e}; timeout flag {fail}; "
          f"recurrences on one XCD (last forward) {same}", flush=True)


if __name__ == "__main__":
    mc = "--mc" in sys.argv[1:]
    a = [int(x) for x in sys.argv[1:] if x != "--mc"]
    shapes = [tuple(a[i:i + 3]) for i in range(0, len(a), 3)] or [(8, 249, 512), (32, 249, 256), (32, 249, 512)]
    for B, T, H in shapes:
        bench(B, T, H, new="mc" if mc else "gru32")
