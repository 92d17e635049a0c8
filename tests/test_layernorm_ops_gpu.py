"""The LayerNorm forward entry points and all eight ln_bwd_k instantiations (csrc/elementwise.hip) against
float64 computed from x, at the shapes where the kernels change path.

MODE bits of the backward: 1 = dx_accum, 2 = dx_accum2, 4 = dx_dropped. What the fused outputs mean
(include/b2p_hip.h, b2p_layernorm_bwd_acc2), with d = dy * mask1 * s1 and gg = d * gamma:

    o          = rstd * (gg - mean_c(gg) - xh * mean_c(gg * xh)) + dx_accum
    dx         = o + dx_accum2
    dx_dropped = o * mask2 * s2            (after dx_accum, before dx_accum2)
    dgamma     = sum_r d * xh,   dbeta = sum_r d,   dbias_in = sum_r dx_dropped
    d16        = bf16(dx_dropped) when dx_dropped is given, else bf16(dx)

The keep masks are the library's own: b2p_dropout of ones over rows * cols elements with the same seed
(dropout_k and the LayerNorm kernels index the mask by the same flat index); each test checks that the
mask's keep share is the binomial one, so an all-ones mask cannot pass. Tolerances are the project's
(test_layernorm_fwd_bwd): 1e-5 forward, 1e-4 gradients; y, dx and dx_dropped per row, relative to the
row's reference maximum.

The test without the gpu marker checks the float64 formulas against autograd."""
import itertools

import pytest
import torch
import torch.nn.functional as F

EPS = 1e-5
TOL_FWD = 1e-5
TOL_BWD = 1e-4
A1, A2, DXD = 1, 2, 4
SEED1, SEED2 = 0x5EED0001, 0x5EED0002

# rows, cols: smallest; rows < 4; cols/4 = 63 and 65 (a partly filled vector slot); the model width; the
# largest cols; nblk = 258 (ln_param_reduce_k's second trip)
SHAPES = ((1, 4), (3, 48), (17, 252), (37, 260), (16, 768), (33, 1024), (4117, 64))
ALL_MODES_AT = ((37, 260), (33, 1024))


def f32_scale(p):
    """The kernels' float 1 / (1 - p), widened to float64."""
    if p <= 0:
        return 1.0
    one = torch.ones((), dtype=torch.float32)
    return float((one / (one - torch.tensor(p, dtype=torch.float32))).double())


def ln_reference(x, gamma, beta, dy, mask1, s1, acc1=None, acc2=None, mask2=None, s2=1.0, eps=EPS):
    """The formulas of the module docstring in the dtype of x (float64 in every use). Absent accumulators
    are zero; dx_dropped and dbias_in are None without mask2."""
    cols = x.shape[1]
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).sum(1) / cols
    rstd = (var + eps).rsqrt()
    xh = (x - mean[:, None]) * rstd[:, None]
    y = mask1 * s1 * (xh * gamma + beta)
    d = dy * mask1 * s1
    gg = d * gamma
    o = rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    if acc1 is not None:
        o = o + acc1
    dx = o if acc2 is None else o + acc2
    dxd = None if mask2 is None else o * mask2 * s2
    return dict(mean=mean, rstd=rstd, y=y, dx=dx, dxd=dxd, dgamma=(d * xh).sum(0), dbeta=d.sum(0),
                dbias=None if dxd is None else dxd.sum(0))


def make_inputs(rows, cols, seed=0, offset=False):
    g = torch.Generator().manual_seed(7919 * rows + 31 * cols + seed)
    x = 30 + 0.5 * torch.randn(rows, cols, generator=g) if offset else torch.randn(rows, cols, generator=g) * 1.5 + 0.3
    return dict(x=x, gamma=torch.randn(cols, generator=g), beta=torch.randn(cols, generator=g),
                dy=torch.randn(rows, cols, generator=g), acc1=torch.randn(rows, cols, generator=g),
                acc2=torch.randn(rows, cols, generator=g))


def row_err(got, ref):
    """max over rows of (the row's largest error / the row's largest reference magnitude)."""
    return float(((got.double() - ref).abs().amax(1) / ref.abs().amax(1).clamp(min=1e-300)).max())


def max_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp(min=1e-300))


# ------------------------------------------------------------------------------------ CPU: the formulas
@pytest.mark.parametrize("rows,cols", [(5, 12), (37, 260)])
def test_formulas_agree_with_autograd_cpu(rows, cols):
    """The float64 formulas against autograd through F.layer_norm, the mask multiplications and the adds:
    x = r + mask2 * s2 * (h + bias) feeds the LayerNorm and a second consumer whose gradient is dx_accum."""
    t = {k: v.double() for k, v in make_inputs(rows, cols, seed=3).items()}
    g = torch.Generator().manual_seed(rows)
    m1 = (torch.rand(rows, cols, generator=g) >= 0.3).double()
    m2 = (torch.rand(rows, cols, generator=g) >= 0.2).double()
    s1, s2 = f32_scale(0.3), f32_scale(0.2)
    h = torch.randn(rows, cols, generator=g).double().requires_grad_(True)
    bias = torch.randn(cols, generator=g).double().requires_grad_(True)
    r = (t["x"] - (m2 * s2 * (h + bias)).detach()).requires_grad_(True)
    gamma, beta = t["gamma"].clone().requires_grad_(True), t["beta"].clone().requires_grad_(True)
    x = r + m2 * s2 * (h + bias)
    y = m1 * s1 * F.layer_norm(x, (cols,), gamma, beta, EPS)
    loss = (y * t["dy"]).sum() + (x * t["acc1"]).sum()
    gr, gh, gbias, gg, gb = torch.autograd.grad(loss, (r, h, bias, gamma, beta))
    ref = ln_reference(x.detach(), t["gamma"], t["beta"], t["dy"], m1, s1, t["acc1"], t["acc2"], m2, s2)
    pairs = dict(y=(ref["y"], y.detach()), dx=(ref["dx"], gr + t["acc2"]), dxd=(ref["dxd"], gh),
                 dgamma=(ref["dgamma"], gg), dbeta=(ref["dbeta"], gb), dbias=(ref["dbias"], gbias))
    for name, (a, b) in pairs.items():
        assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max())), name
    # without the optional terms the same function is plain LayerNorm
    ones = torch.ones(rows, cols, dtype=torch.float64)
    xr = t["x"].clone().requires_grad_(True)
    yr = F.layer_norm(xr, (cols,), t["gamma"], t["beta"], EPS)
    (gx,) = torch.autograd.grad(yr, xr, t["dy"])
    ref0 = ln_reference(t["x"], t["gamma"], t["beta"], t["dy"], ones, 1.0)
    assert float((ref0["y"] - yr.detach()).abs().max()) <= 1e-10 and float((ref0["dx"] - gx).abs().max()) <= 1e-10
    assert ref0["dxd"] is None and ref0["dbias"] is None


# ------------------------------------------------------------------------------------ GPU
def _call(name, *args):
    from wav2vec2forbrain_amd import functional as Fn
    Fn._lib.call(name, *args, Fn._lib.stream_ptr())


def P(t):
    return None if t is None else t.data_ptr()


def keep_mask(rows, cols, p, seed):
    """The library's keep mask over the flat index (float64 0 / 1 on the CPU), from b2p_dropout of ones;
    its keep share must lie within 5 binomial standard deviations of 1 - p."""
    n = rows * cols
    if p <= 0:
        return torch.ones(rows, cols, dtype=torch.float64)
    ones = torch.ones(n, device="cuda")
    out = torch.empty_like(ones)
    _call("b2p_dropout", P(ones), P(out), n, float(p), seed)
    torch.cuda.synchronize()
    mask = (out != 0).view(rows, cols).cpu()
    assert bool((out[out != 0] == torch.tensor(f32_scale(p), dtype=torch.float32)).all())
    share = float(mask.double().mean())
    assert abs(share - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, (share, n)
    return mask.double()


def ln_fwd(t, drop_p=0.0, seed=0, entry="fwd"):
    """One forward launch. entry: 'fwd' (y), 'fwd16' (y, bf16 y16), 'x16h' / 'x16b' (y, fp16 or bf16 y16, bf16
    y16b; no dropout). Returns (y, mean, rstd, y16, y16b)."""
    x, gamma, beta = t["x"].cuda(), t["gamma"].cuda(), t["beta"].cuda()
    rows, cols = x.shape
    y = torch.full_like(x, float("nan"))
    mean, rstd = torch.full((rows,), float("nan"), device="cuda"), torch.full((rows,), float("nan"), device="cuda")
    y16 = y16b = None
    if entry == "fwd":
        _call("b2p_layernorm_fwd", P(x), P(gamma), P(beta), P(y), P(mean), P(rstd), rows, cols, EPS, float(drop_p), seed)
    elif entry == "fwd16":
        y16 = torch.zeros(rows, cols, device="cuda", dtype=torch.bfloat16)
        _call("b2p_layernorm_fwd16", P(x), P(gamma), P(beta), P(y), P(y16), P(mean), P(rstd), rows, cols, EPS,
              float(drop_p), seed)
    else:
        assert drop_p == 0.0
        half = entry == "x16h"
        y16 = torch.zeros(rows, cols, device="cuda", dtype=torch.float16 if half else torch.bfloat16)
        y16b = torch.zeros(rows, cols, device="cuda", dtype=torch.bfloat16)
        _call("b2p_layernorm_fwd_x16", P(x), P(gamma), P(beta), P(y), P(y16), int(half), P(y16b), P(mean), P(rstd),
              rows, cols, EPS)
    torch.cuda.synchronize()
    return y, mean, rstd, y16, y16b


def ln_bwd(t, mean, rstd, mode, drop_p, in_drop_p, want_d16, lazy=False):
    """b2p_layernorm_bwd_gated with NULL gates (the kernel behind every backward entry point), on the
    statistics the forward saved. Returns dict(dx, dxd, d16, dgamma, dbeta, dbias, ws, nblk), absent -> None."""
    from wav2vec2forbrain_amd import _lib
    x, gamma, dy = t["x"].cuda(), t["gamma"].cuda(), t["dy"].cuda()
    rows, cols = x.shape
    nan = float("nan")
    acc1 = t["acc1"].cuda() if mode & A1 else None
    acc2 = t["acc2"].cuda() if mode & A2 else None
    dx = torch.full_like(x, nan)
    dxd = torch.full_like(x, nan) if mode & DXD else None
    d16 = torch.zeros(rows, cols, device="cuda", dtype=torch.bfloat16) if want_d16 else None
    dg, db = (None, None) if lazy else (torch.full((cols,), nan, device="cuda"), torch.full((cols,), nan, device="cuda"))
    dbi = torch.full((cols,), nan, device="cuda") if (mode & DXD) and not lazy else None
    ws = torch.full((int(_lib.load().b2p_layernorm_bwd_workspace(rows, cols)),), nan, device="cuda")
    _call("b2p_layernorm_bwd_gated", P(dy), P(x), P(gamma), P(mean), P(rstd), P(dx), P(dg), P(db), rows, cols, P(acc1),
          P(acc2), float(drop_p), SEED1, P(dxd), float(in_drop_p), SEED2, P(dbi), P(d16), None, None, P(ws))
    torch.cuda.synchronize()
    return dict(dx=dx, dxd=dxd, d16=d16, dgamma=dg, dbeta=db, dbias=dbi, ws=ws, nblk=-(-rows // 16))


def _reference(t, mode, drop_p, in_drop_p):
    rows, cols = t["x"].shape
    m1 = keep_mask(rows, cols, drop_p, SEED1)
    m2 = keep_mask(rows, cols, in_drop_p, SEED2) if mode & DXD else None
    d = {k: v.double() for k, v in t.items()}
    ref = ln_reference(d["x"], d["gamma"], d["beta"], d["dy"], m1, f32_scale(drop_p), d["acc1"] if mode & A1 else None,
                       d["acc2"] if mode & A2 else None, m2, f32_scale(in_drop_p),
                       eps=float(torch.tensor(EPS, dtype=torch.float32).double()))
    return ref, m1, m2


def _check_fwd(got, ref, m1, tol=TOL_FWD):
    y, mean, rstd = got[0].cpu(), got[1].cpu(), got[2].cpu()
    assert bool(torch.isfinite(y).all())
    # the mean's error is absolute in the scale of the row's entries; rstd's is relative
    xmax = ref["xmax"]
    errs = dict(mean=float(((mean.double() - ref["mean"]).abs() / xmax).max()),
                rstd=float(((rstd.double() - ref["rstd"]).abs() / ref["rstd"]).max()), y=row_err(y, ref["y"]))
    for k, v in errs.items():
        assert v <= tol, (k, v)
    assert bool((y[m1 == 0] == 0).all()) and bool((y[m1 != 0] != 0).all())
    return errs


def _check_bwd(out, ref, mode, m2, tol=TOL_BWD):
    cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()}
    errs = dict(dx=row_err(cpu["dx"], ref["dx"]), dgamma=max_err(cpu["dgamma"], ref["dgamma"]),
                dbeta=max_err(cpu["dbeta"], ref["dbeta"]))
    if mode & DXD:
        dxd = cpu["dxd"]
        errs["dxd"] = row_err(dxd, ref["dxd"])
        errs["dbias"] = max_err(cpu["dbias"], ref["dbias"])
        assert bool((dxd[m2 == 0] == 0).all())
        # dbias_in is the column sum of the dx_dropped the kernel wrote
        own = dxd.double().sum(0)
        assert float((cpu["dbias"].double() - own).abs().max()) <= 1e-6 * float(own.abs().max())
    else:
        assert cpu["dxd"] is None and cpu["dbias"] is None
    for k, v in errs.items():
        assert v <= tol, (k, v, mode)
    if cpu["d16"] is not None:
        src = cpu["dxd"] if mode & DXD else cpu["dx"]
        assert torch.equal(cpu["d16"], src.bfloat16()), mode
    return errs


def _bwd_cases():
    cases = []
    for (rows, cols), mode, d16 in itertools.product(ALL_MODES_AT, range(8), (False, True)):
        cases.append((rows, cols, mode, 0.1, 0.1, d16))
    for rows, cols in SHAPES:
        if (rows, cols) not in ALL_MODES_AT:
            cases += [(rows, cols, 0, 0.1, 0.1, True), (rows, cols, 7, 0.1, 0.1, True)]
    cases.append((37, 260, 7, 0.0, 0.1, True))       # no output dropout: the mask code is skipped
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,mode,drop_p,in_drop_p,d16", _bwd_cases())
def test_ln_bwd_modes(rows, cols, mode, drop_p, in_drop_p, d16):
    """Forward (with the output dropout) then the backward instantiation `mode`, both against float64."""
    t = make_inputs(rows, cols, seed=mode)
    ref, m1, m2 = _reference(t, mode, drop_p, in_drop_p)
    ref["xmax"] = t["x"].double().abs().amax(1)
    fwd = ln_fwd(t, drop_p, SEED1)
    _check_fwd(fwd, ref, m1)
    out = ln_bwd(t, fwd[1], fwd[2], mode, drop_p, in_drop_p, d16)
    _check_bwd(out, ref, mode, m2)
    assert bool(torch.isfinite(out["dx"]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_ln_fwd_entry_points(rows, cols):
    """b2p_layernorm_fwd / _fwd16 (with and without dropout) and _fwd_x16 (fp16 and bf16 y16, bf16 y16b):
    the same fp32 y bit for bit, and each 16-bit copy the rounding of it."""
    t = make_inputs(rows, cols, seed=11)
    for drop_p in (0.0, 0.1):
        ref, m1, _ = _reference(t, 0, drop_p, 0.0)
        ref["xmax"] = t["x"].double().abs().amax(1)
        base = ln_fwd(t, drop_p, SEED1, "fwd")
        _check_fwd(base, ref, m1)
        entries = ("fwd16",) if drop_p else ("fwd16", "x16h", "x16b")
        for entry in entries:
            y, mean, rstd, y16, y16b = ln_fwd(t, drop_p, SEED1, entry)
            assert torch.equal(y, base[0]) and torch.equal(mean, base[1]) and torch.equal(rstd, base[2]), entry
            assert torch.equal(y16, y.half() if entry == "x16h" else y.bfloat16()), entry
            if y16b is not None:
                assert torch.equal(y16b, y.bfloat16()), entry


@pytest.mark.gpu
def test_ln_bwd_dropped_dy_contributes_exact_zero():
    """One row, one block: dbeta is d itself and dgamma is d * xh, so both are exactly 0 at every column the
    output dropout dropped (d is selected, not scaled towards 0), and dy * s1 elsewhere."""
    rows, cols = 1, 260
    t = make_inputs(rows, cols, seed=5)
    ref, m1, _ = _reference(t, 0, 0.1, 0.0)
    assert 0 < int((m1 == 0).sum()) < cols
    fwd = ln_fwd(t, 0.1, SEED1)
    out = ln_bwd(t, fwd[1], fwd[2], 0, 0.1, 0.0, False)
    db, dg = out["dbeta"].cpu(), out["dgamma"].cpu()
    drop = m1[0] == 0
    assert bool((db[drop] == 0).all()) and bool((dg[drop] == 0).all())
    assert torch.equal(db[~drop], (t["dy"][0] * torch.tensor(f32_scale(0.1), dtype=torch.float32))[~drop])


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(37, 260), (4117, 64)])
def test_ln_bwd_lazy_partials(rows, cols):
    """dgamma = dbeta = dbias_in = NULL leaves [3][nblk][cols] block partials in the workspace: their
    float64 sums over the blocks are the direct outputs; dx, dx_dropped and d16 do not change."""
    t = make_inputs(rows, cols, seed=7)
    fwd = ln_fwd(t, 0.1, SEED1)
    direct = ln_bwd(t, fwd[1], fwd[2], 7, 0.1, 0.1, True)
    lazy = ln_bwd(t, fwd[1], fwd[2], 7, 0.1, 0.1, True, lazy=True)
    for k in ("dx", "dxd", "d16"):
        assert torch.equal(lazy[k], direct[k]), k
    nblk = lazy["nblk"]
    parts = lazy["ws"][:3 * nblk * cols].view(3, nblk, cols).cpu().double()
    assert bool(torch.isfinite(parts).all())
    for q, k in enumerate(("dgamma", "dbeta", "dbias")):
        want = direct[k].cpu().double()
        assert float((parts[q].sum(0) - want).abs().max()) <= 1e-6 * float(want.abs().max()), k


@pytest.mark.gpu
def test_ln_offset_input():
    """x = 30 + 0.5 * randn: fp32 loses digits in x - mean whatever the kernel does, so the bound is 8 times
    the error of torch's fp32 CPU LayerNorm and its autograd against float64 on the same inputs, and never
    below the project's tolerance."""
    rows, cols = 37, 768
    t = make_inputs(rows, cols, seed=9, offset=True)
    ref, m1, _ = _reference(t, 0, 0.0, 0.0)
    xmax = ref["xmax"] = t["x"].double().abs().amax(1)
    # the fp32 CPU baseline, in the same error measures
    xr = t["x"].clone().requires_grad_(True)
    gr, br = t["gamma"].clone().requires_grad_(True), t["beta"].clone().requires_grad_(True)
    y32, mean32, rstd32 = torch.native_layer_norm(xr, (cols,), gr, br, EPS)
    gx, gg, gb = torch.autograd.grad(y32, (xr, gr, br), t["dy"])
    base = dict(mean=float(((mean32.detach().view(rows).double() - ref["mean"]).abs() / xmax).max()),
                rstd=float(((rstd32.detach().view(rows).double() - ref["rstd"]).abs() / ref["rstd"]).max()),
                y=row_err(y32.detach(), ref["y"]), dx=row_err(gx, ref["dx"]), dgamma=max_err(gg, ref["dgamma"]),
                dbeta=max_err(gb, ref["dbeta"]))
    fwd = ln_fwd(t)
    out = ln_bwd(t, fwd[1], fwd[2], 0, 0.0, 0.0, False)
    got = dict(_check_fwd(fwd, ref, m1, tol=float("inf")))
    got.update(_check_bwd(out, ref, 0, None, tol=float("inf")))
    ratios = {k: got[k] / max(base[k], 1e-300) for k in got}
    print("layernorm offset input: kernel error / fp32 CPU baseline error: "
          + ", ".join(f"{k} {got[k]:.2e} / {base[k]:.2e} = {ratios[k]:.2f}" for k in got))
    for k in got:
        floor = TOL_FWD if k in ("mean", "rstd", "y") else TOL_BWD
        assert got[k] <= max(floor, 8 * base[k]), (k, got[k], base[k])
