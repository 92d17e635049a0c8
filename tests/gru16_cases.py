"""What tests/test_gru16_step_gpu.py and tests/test_gru16_step_host.py share for the 16-bit persistent GRU
recurrences: csrc/gru16.hip (gru16_fwd / gru16_bwd<H>, H = 32, 64, 128, 256, one CU per recurrence, lane-native
tensors) and csrc/grumc.hip (grumc_fwd / grumc_bwd<H>, H = 256, 384, 512, 1024, H / 64 CUs per recurrence).

Teacher-forced steps. Both kernels store h of every step and (r, z, n, W_hn h + b_hn) of every step, the backward
dgi and dgh of every step, so every time step is checked on its own from the kernel's own previous step: the
reference rounds the kernel's fp32 h_{s-1} to fp16 (the backward: the kernel's fp32 dgh_{s+1} to bf16), which is
what the kernel's LDS image / exchange granule holds, and evaluates the step in float64. What is left between the
two is fp32 accumulation and the fast sigm / tanh_fast of csrc/gru_dev.h; nothing builds up over T and a fault at
one step is not damped by later ones. All arrays here are in PROCESSING order: (ndir, T, B, ...) with index s the
direction's own step (t = s for d = 0, T - 1 - s for d = 1); proc() / std() convert from / to the standard
(B, T, ndir * R * H) layout.

Read in the kernels (the 16-bit image is the rounding of the very fp32 value stored):
  gru16_fwd   finish(): b2p_pack_f16x4(hh) into the next LDS image and bst4(h_r, hh) take the same four hh; the
              h0 image is b2p_pack_f16x4 of the h0 values kept in hp. saved[3] is the accumulator acc[ub][2] =
              b_hn + W_hn h. b_hr / b_hz are NOT read: the caller folds them into gi (kernel_gi()).
  gru16_bwd   store_bf16x4(ar, az, an * r) beside bst4(dg_r, ..., ar / az / mul4(a4, rv)): the same products.
  grumc_fwd   pack2h(hh[0], hh[1]) in put_granule beside st_h = hh; all of b_hh is added in the kernel
              (acc = gi + b_hh for r, z; b_hn for n), in fp32 before the MFMAs.
  grumc_bwd   dgh_granule(st_ar, st_az, st_an * st_r) beside store_out's dgh = (st_ar, st_az, st_an * st_r).
Neither kernel differs from the rule; padded batch rows (b >= B) carry h = 0 and dgh = 0 and are never stored
(grumc) or stored as 0 in the lane-native padding (gru16).

ref_fwd64 / ref_bwd64: the step in float64 (the dh chain of the backward is carried in float64; the z h_{s-1}
term uses the unrounded fp32 h_{s-1}, as the kernels do). restate32: the same step in numpy float32: 16-bit
operands, fp32 accumulation in chained 32-wide blocks (a block's 32 products are summed exactly and the running sum
is rounded to fp32 once per block; gru16_bwd: gate rows in the order r, z, n; grumc_bwd: k = 3 * unit + gate in
two chains of even and odd blocks), __expf(x) = exp2(float32(x * log2e)), sigm and tanh_fast spelled as in
gru_dev.h. It runs freely (its own h and dgh feed its next step) and is the calibration side of the gate; it also
carries the planted defects of the host test.

The gate, per output (h, r, z, n, ghn, dgi, dgh, dh0) and case:

    E_k <= 4 * E_r + 2 * 2^-24 * max|ref64|

E_k = max |kernel - ref64(kernel's own h, saved, dgh)|, E_r = max |restate32 - ref64(restate32's own h, saved,
dgh)| on the same inputs. 4 = 2 (the project's allowance for the same sums in another order, tests/
test_gru32_gpu.py, tests/test_attn32_gpu.py) x 2 (the matrix unit's accumulator and the hardware exp2 / rcp are
charged a whole ulp each in tests/attn16_cases.py, UA = 2^-23; numpy rounds to half an ulp). Nothing is fitted to
the kernels.

Inputs: a generator seeded by (H, B, T); gi = randn, whh = randn / sqrt(H), bhh = 0.1 randn, h0 = randn, dout =
randn; twelve gi entries spread over rows, steps, directions and all three gates are set to +-20 and +-90, which
saturate sigm / tanh_fast (__expf overflows to inf and underflows to 0): every output must stay finite.
"""
import functools
import math
import types

import numpy as np

F32, F64 = np.float32, np.float64
BG = 16
LOG2E32 = np.float32(1.0 / math.log(2.0))
H_GRU16 = (32, 64, 128, 256)
H_MC = (256, 384, 512, 1024)
OUTS = ("h", "r", "z", "n", "ghn", "dgi", "dgh", "dh0")
FACTOR, ULPS = 4.0, 2.0 * 2.0 ** -24

# (B, T, ndir, h0, bhh)
CASES_GRU16 = [(1, 1, 2, True, True),      # T = 1: only the tail of the loop unrolled by two
               (15, 2, 2, False, True),    # NULL h0 / dh0 through the zero-size buffer resource
               (16, 3, 1, True, False),    # NULL bhh, one direction
               (17, 4, 2, True, True),     # a second batch group that holds one row
               (33, 41, 2, True, True)]
CASES_MC = [(5, 1, 2, True, True), (17, 2, 2, False, True), (17, 3, 1, True, False), (33, 41, 2, True, True)]
CASE_MC_WIDE = (65, 3, 2, False, True)     # H = 512, 1024 (there: the chunked launch)
ISOLATION = (17, 3, 2, True, True)         # batch row 1 poisoned


def mc_cases(H):
    return CASES_MC + ([CASE_MC_WIDE] if H in (512, 1024) else [])


# ------------------------------------------------------------------------------------------------ roundings
def r16(x):
    """fp32 -> fp16 (round to nearest even, saturating as b2p_f16_bits) -> fp32."""
    return np.clip(np.asarray(x, F32), -65504.0, 65504.0).astype(np.float16).astype(F32)


def rbf(x):
    """fp32 -> bf16 (round to nearest even) -> fp32; finite input."""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(F32)


# ------------------------------------------------------------------------------------------ lane-native layout
def ln_floats(B, T, H, nd, R):
    return nd * (-(-B // BG)) * BG * T * H * R


def _nib(rmap, k):
    return (rmap >> (4 * k)) & 15


def ln_permute_loops(src, dst, B, T, H, nd, Rl, Rs, rmap, to_lane):
    """The lane-native index formula of csrc/gru16.hip's header comment as plain loops (in place on dst).
    LN float offset = (((((d*NBG + bg)*T + s)*U + ub)*R + r)*64 + lane)*4 + i, lane = (b % 16) + 16*((j % 16) / 4),
    i = j % 4, ub = j / 16, U = H / 16, s = t (d = 0) or T - 1 - t. LN record r <-> standard record nibble r of
    rmap (15: not mapped); to_lane writes 0 into padded rows, from-lane skips them."""
    U, NBG = H // 16, -(-B // BG)
    S = src.reshape(-1)
    D = dst.reshape(-1)
    for d in range(nd):
        for bg in range(NBG):
            for s in range(T):
                t = s if d == 0 else T - 1 - s
                for ub in range(U):
                    for r in range(Rl):
                        rs = _nib(rmap, r)
                        if rs == 15:
                            continue
                        for lane in range(64):
                            b = bg * BG + lane % 16
                            for i in range(4):
                                j = ub * 16 + 4 * (lane // 16) + i
                                ln = (((((d * NBG + bg) * T + s) * U + ub) * Rl + r) * 64 + lane) * 4 + i
                                so = ((b * T + t) * nd + d) * Rs * H + rs * H + j
                                if to_lane:
                                    D[ln] = S[so] if b < B else 0.0
                                elif b < B:
                                    D[so] = S[ln]
    return dst


def ln_index(B, T, H, nd, Rl, Rs, rmap):
    """Vectorised form: for every LN float its standard flat index, whether its row exists, and whether its record
    is mapped."""
    U, NBG = H // 16, -(-B // BG)
    d, bg, s, ub, r, lane, i = np.ogrid[:nd, :NBG, :T, :U, :Rl, :64, :4]
    b = bg * BG + lane % 16
    j = ub * 16 + 4 * (lane // 16) + i
    t = np.where(d == 0, s, T - 1 - s)
    rs = np.array([_nib(rmap, k) for k in range(Rl)])[r]
    so = ((b * T + t) * nd + d) * Rs * H + rs * H + j
    shape = (nd, NBG, T, U, Rl, 64, 4)
    mapped = np.broadcast_to(rs != 15, shape).reshape(-1)
    row = np.broadcast_to(b < B, shape).reshape(-1)
    return np.broadcast_to(so, shape).reshape(-1), row, mapped


def ln_permute(src, dst, B, T, H, nd, Rl, Rs, rmap, to_lane):
    so, row, mapped = ln_index(B, T, H, nd, Rl, Rs, rmap)
    S, D = src.reshape(-1), dst.reshape(-1)
    ok = row & mapped
    if to_lane:
        D[mapped & ~row] = 0.0
        D[ok] = S[so[ok]]
    else:
        D[so[ok]] = S[ok]
    return dst


# ---------------------------------------------------------------------------------------------------- inputs
def proc(x, nd, R):
    """(B, T, nd*R*H) -> (nd, T, B, R, H) in processing order."""
    B, T = x.shape[:2]
    y = x.reshape(B, T, nd, R, -1).transpose(2, 1, 0, 3, 4).copy()
    if nd == 2:
        y[1] = y[1, ::-1].copy()
    return y


def std(y):
    """(nd, T, B, R, H) in processing order -> (B, T, nd*R*H)."""
    nd, T, B = y.shape[:3]
    y = y.copy()
    if nd == 2:
        y[1] = y[1, ::-1].copy()
    return np.ascontiguousarray(y.transpose(2, 1, 0, 3, 4)).reshape(B, T, -1)


@functools.lru_cache(maxsize=None)
def case(H, B, T, nd, has_h0, has_bias):
    """The fp32 inputs of one shape in the standard layouts; computed once, never modified."""
    g = np.random.default_rng((H, B, T))
    rn = lambda *s: g.standard_normal(s).astype(F32)
    gi = rn(B, T, nd * 3 * H)
    whh = (rn(nd, 3 * H, H) / np.float32(math.sqrt(H))).astype(F32)
    bhh = (rn(nd, 3 * H) * np.float32(0.1)).astype(F32)
    h0 = rn(nd, B, H)
    dout = rn(B, T, nd * H)
    vals = (20.0, -20.0, 90.0, -90.0)
    for k in range(12):     # k % 3 and k % 4 pair every gate with every value
        b, t, d, j = (5 * k + 1) % B, (7 * k + 2) % T, k % nd, (37 * k + 5) % H
        gi[b, t, d * 3 * H + (k % 3) * H + j] = vals[k % 4]
    c = types.SimpleNamespace(H=H, B=B, T=T, nd=nd, gi=gi, whh=whh, bhh=bhh if has_bias else None,
                              h0=h0 if has_h0 else None, dout=dout)
    for a in (gi, whh, bhh, h0, dout):
        a.setflags(write=False)
    return c


def kernel_gi(c, backend):
    """The gi the back-end is handed: gru16 takes b_hr and b_hz folded in by the caller (fp32), grumc the plain gi."""
    if backend == "mc" or c.bhh is None:
        return c.gi
    f = c.bhh.reshape(c.nd, 3, c.H).copy()
    f[:, 2] = 0
    return (c.gi + f.reshape(1, 1, -1)).astype(F32)


def _terms(c, backend):
    """(gi in processing order as the kernel receives it, the biases the kernel itself adds (nd, 3, H), dout)."""
    bias = np.zeros((c.nd, 3, c.H), F32) if c.bhh is None else c.bhh.reshape(c.nd, 3, c.H).copy()
    if backend == "gru16":
        bias[:, :2] = 0
    return proc(kernel_gi(c, backend), c.nd, 3), bias, proc(c.dout, c.nd, 1)[:, :, :, 0]


def _hprev(c, h):
    """h_{s-1} of every step (nd, T, B, H) from h of every step and h0 (or 0), in h's dtype."""
    h0 = np.zeros((c.nd, c.B, c.H), h.dtype) if c.h0 is None else c.h0.astype(h.dtype)
    return np.concatenate([h0[:, None], h[:, :-1]], 1)


# ------------------------------------------------------------------------------------------ float64 references
def _sig64(x):
    return 1.0 / (1.0 + np.exp(-x))


def ref_fwd64(c, backend, h):
    """Every step in float64 from fp16(h_{s-1}) of the h handed in (fp32, (nd, T, B, H)) and fp16(W_hh)."""
    gi, bias, _ = _terms(c, backend)
    gi, bias = gi.astype(F64), bias.astype(F64)
    hp = _hprev(c, np.asarray(h, F32))
    W = r16(c.whh).astype(F64)                                               # (nd, 3H, H)
    gh = r16(hp).astype(F64).reshape(c.nd, c.T * c.B, c.H) @ W.transpose(0, 2, 1)
    gh = gh.reshape(c.nd, c.T, c.B, 3, c.H) + bias[:, None, None]
    with np.errstate(over="ignore"):
        r = _sig64(gi[..., 0, :] + gh[..., 0, :])
        z = _sig64(gi[..., 1, :] + gh[..., 1, :])
    ghn = gh[..., 2, :]
    n = np.tanh(gi[..., 2, :] + r * ghn)
    return {"h": (1.0 - z) * n + z * hp.astype(F64), "r": r, "z": z, "n": n, "ghn": ghn}


def ref_bwd64(c, backend, h, sav, dgh):
    """Every backward step in float64 from the forward outputs handed in (h (nd, T, B, H), sav (nd, T, B, 4, H),
    fp32) and bf16(dgh_{s+1}) of the dgh handed in ((nd, T, B, 3, H), fp32); the dh chain in float64."""
    _, _, do = _terms(c, backend)
    nd, T, B, H = c.nd, c.T, c.B, c.H
    hp = _hprev(c, np.asarray(h, F32)).astype(F64)
    W = rbf(c.whh).astype(F64)                                               # (nd, 3H, H)
    rec = (rbf(dgh).astype(F64).reshape(nd, T * B, 3 * H) @ W).reshape(nd, T, B, H)   # W^T dgh_s
    sv = np.asarray(sav, F64)
    r, z, n, g = (sv[:, :, :, q] for q in range(4))
    dgi, dg = np.zeros((nd, T, B, 3, H)), np.zeros((nd, T, B, 3, H))
    dh = np.zeros((nd, B, H))
    for s in range(T - 1, -1, -1):
        dh = do[:, s].astype(F64) + (rec[:, s + 1] + z[:, s + 1] * dh if s < T - 1 else 0.0)
        dn = dh * (1.0 - z[:, s])
        dz = dh * (hp[:, s] - n[:, s])
        dan = dn * (1.0 - n[:, s] ** 2)
        dar = dan * g[:, s] * r[:, s] * (1.0 - r[:, s])
        daz = dz * z[:, s] * (1.0 - z[:, s])
        dgi[:, s] = np.stack([dar, daz, dan], 2)
        dg[:, s] = np.stack([dar, daz, dan * r[:, s]], 2)
    return {"dgi": dgi, "dgh": dg, "dh0": rec[:, 0] + z[:, 0] * dh}


# ---------------------------------------------------------------------------------------- float32 restatement
DEFECTS = ("h_fp16", "bf16_fwd", "w_unrounded", "dgh_unrounded", "dh_bf16", "drop_kstep", "stale_block", "no_bhn",
           "sav3_no_bhn")


def _expf(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2((x * LOG2E32).astype(F32)).astype(F32)


def sigm(x):
    return (F32(1) / (F32(1) + _expf(-x))).astype(F32)


def tanh_fast(x):
    return (F32(1) - F32(2) * (F32(1) / (F32(1) + _expf(F32(2) * x)))).astype(F32)


def _wblocks(Wkn):
    """(K, N) fp32 -> (K/32, 32, N) float64."""
    return Wkn.astype(F64).reshape(Wkn.shape[0] // 32, 32, Wkn.shape[1])


def _blockdots(x, Wb):
    """x (B, K) fp32, Wb (K/32, 32, N): the exact sums of each 32-wide block's products, (K/32, B, N) float64."""
    return x.astype(F64).reshape(x.shape[0], Wb.shape[0], 32).transpose(1, 0, 2) @ Wb


def _chain(acc, bd, idx):
    for i in idx:
        acc = (acc.astype(F64) + bd[i]).astype(F32)
    return acc


def restate32(c, backend, defect=None):
    """The free-running fp32 restatement of forward and backward: dict h, sav, dgi, dgh, dh0 (None without h0)."""
    assert defect is None or defect in DEFECTS
    nd, T, B, H = c.nd, c.T, c.B, c.H
    gi, bias, do = _terms(c, backend)
    rf = rbf if defect == "bf16_fwd" else r16
    rw = (lambda w: w) if defect == "w_unrounded" else None
    h = np.zeros((nd, T, B, H), F32)
    sav = np.zeros((nd, T, B, 4, H), F32)
    dgi = np.zeros((nd, T, B, 3, H), F32)
    dgh = np.zeros((nd, T, B, 3, H), F32)
    dh0 = np.zeros((nd, B, H), F32)
    for d in range(nd):
        Wf = _wblocks((rw or rf)(c.whh[d]).T)                        # K = H, N = 3H (gate-major)
        bn = np.zeros(H, F32) if defect == "no_bhn" else bias[d, 2]
        hp = np.zeros((B, H), F32) if c.h0 is None else c.h0[d].copy()
        imgs = [rf(hp)]
        for s in range(T):
            img = imgs[s]
            if defect == "stale_block" and s >= 1:                   # one member's 64 units one step late
                img = img.copy()
                img[:, :64] = imgs[s - 1][:, :64]
            bd = _blockdots(img, Wf)
            if defect == "drop_kstep":                               # units 16..31 of every gate miss k-step 0
                bd[0].reshape(B, 3, H)[:, :, 16:32] = 0.0
            acc = np.concatenate([gi[d, s, :, 0] + bias[d, 0], gi[d, s, :, 1] + bias[d, 1],
                                  np.broadcast_to(bn, (B, H))], 1).astype(F32)
            acc = _chain(acc, bd, range(bd.shape[0])).reshape(B, 3, H)
            r, z = sigm(acc[:, 0]), sigm(acc[:, 1])
            n = tanh_fast(gi[d, s, :, 2] + r * acc[:, 2])
            hh = ((F32(1) - z) * n + z * hp).astype(F32)
            h[d, s] = hh
            sav[d, s] = np.stack([r, z, n, acc[:, 2] - bias[d, 2] if defect == "sav3_no_bhn" else acc[:, 2]], 1)
            hp = r16(hh) if defect == "h_fp16" else hh
            imgs.append(rf(hh))
        # backward
        Wk = (rw or rbf)(c.whh[d])                                    # (3H, H): K = 3H
        if backend == "mc":                                           # k = 3 * unit + gate
            Wk = Wk.reshape(3, H, H).transpose(1, 0, 2).reshape(3 * H, H)
        Wt = _wblocks(np.ascontiguousarray(Wk))
        nb = Wt.shape[0]

        def recur(g3):                                                # g3 (B, 3, H) fp32 dgh of the later step
            x = g3 if defect == "dgh_unrounded" else rbf(g3)
            x = x.transpose(0, 2, 1).reshape(B, 3 * H) if backend == "mc" else x.reshape(B, 3 * H)
            bd = _blockdots(np.ascontiguousarray(x), Wt)
            zero = np.zeros((B, H), F32)
            if backend == "mc":
                return (_chain(zero, bd, range(0, nb, 2)) + _chain(zero, bd, range(1, nb, 2))).astype(F32)
            return _chain(zero, bd, range(nb))

        hprev = _hprev(c, h)[d]
        dhn, zn = np.zeros((B, H), F32), np.zeros((B, H), F32)
        for s in range(T - 1, -1, -1):
            r, z, n, g = (sav[d, s, :, q] for q in range(4))
            if s == T - 1:
                dh = do[d, s].copy()
            elif backend == "mc":
                dh = (do[d, s] + (recur(dgh[d, s + 1]) + zn * dhn)).astype(F32)
            else:
                dh = ((do[d, s] + recur(dgh[d, s + 1])) + zn * dhn).astype(F32)
            dn = dh * (F32(1) - z)
            dz = dh * (hprev[s] - n)
            dan = (dn * (F32(1) - n * n)).astype(F32)
            dar = (dan * g * r * (F32(1) - r)).astype(F32)
            daz = (dz * z * (F32(1) - z)).astype(F32)
            dgi[d, s] = np.stack([dar, daz, dan], 1)
            dgh[d, s] = np.stack([dar, daz, (dan * r).astype(F32)], 1)
            dhn, zn = rbf(dh) if defect == "dh_bf16" else dh, z
        dh0[d] = (recur(dgh[d, 0]) + zn * dhn).astype(F32)
    return {"h": h, "sav": sav, "dgi": dgi, "dgh": dgh, "dh0": dh0 if c.h0 is not None else None}


# ------------------------------------------------------------------------------------------------- the gate
def errors(c, backend, got):
    """{output: (max |got - ref64 of got's own previous steps|, max |ref64|)}; dh0 only where the case has h0.
    Raises AssertionError if an output is not finite."""
    rf = ref_fwd64(c, backend, got["h"])
    rb = ref_bwd64(c, backend, got["h"], got["sav"], got["dgh"])
    mine = {"h": got["h"], "r": got["sav"][:, :, :, 0], "z": got["sav"][:, :, :, 1], "n": got["sav"][:, :, :, 2],
            "ghn": got["sav"][:, :, :, 3], "dgi": got["dgi"], "dgh": got["dgh"], "dh0": got["dh0"]}
    out = {}
    for name in OUTS:
        if mine[name] is None:
            assert name == "dh0" and c.h0 is None
            continue
        ref = rf[name] if name in rf else rb[name]
        assert mine[name].shape == ref.shape, (name, mine[name].shape, ref.shape)
        assert np.isfinite(mine[name]).all(), f"{name}: not finite"
        out[name] = (float(np.abs(mine[name].astype(F64) - ref).max()), float(np.abs(ref).max()))
    return out


@functools.lru_cache(maxsize=None)
def restate_errors(backend, H, B, T, nd, has_h0, has_bias):
    """E_r of one case: restate32 against the references fed with restate32's own h, saved and dgh."""
    c = case(H, B, T, nd, has_h0, has_bias)
    return errors(c, backend, restate32(c, backend))


def gate(e_k, e_r, refmax):
    return FACTOR * e_r + ULPS * refmax


def judge(tag, ek, er):
    """Prints E_k, E_r, their ratio and the gate per output; returns ({output: E_k / E_r}, the outputs past the
    gate)."""
    ratios, fails = {}, []
    for name, (e_k, refmax) in ek.items():
        e_r = er[name][0]
        lim = gate(e_k, e_r, refmax)
        ratios[name] = e_k / e_r if e_r > 0 else (0.0 if e_k == 0 else float("inf"))
        print(f"{tag} {name}: E_k {e_k:.3e} E_r {e_r:.3e} ratio {ratios[name]:.2f} gate {lim:.3e} max|ref| {refmax:.3g}")
        if not e_k <= lim:
            fails.append((name, e_k, e_r, lim))
    return ratios, fails


# -------------------------------------------------------------------------------------------------- GPU runs
GUARD = 1024    # floats in front of and behind every output (a multiple of 16 bytes)


def _lib():
    from wav2vec2forbrain_amd import _lib
    return _lib


class Guarded:
    """Views between NaN guard rows; check(): guards untouched, every view fully written with finite values."""

    def __init__(self):
        self.all = []

    def new(self, n):
        import torch
        whole = torch.full((int(n) + 2 * GUARD,), float("nan"), device="cuda")
        view = whole[GUARD:GUARD + int(n)]
        assert view.data_ptr() % 16 == 0
        self.all.append((whole, view))
        return view

    def check(self, finite=True):
        import torch
        for whole, view in self.all:
            assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[GUARD + view.numel():]).all())
            if finite:
                assert bool(torch.isfinite(view).all())


def _device_inputs(c, backend, poison_row):
    import torch
    gi = torch.from_numpy(np.array(kernel_gi(c, backend))).cuda()
    dout = torch.from_numpy(np.array(c.dout)).cuda()
    h0 = None if c.h0 is None else torch.from_numpy(np.array(c.h0)).cuda()
    if poison_row is not None:
        gi[poison_row] = float("nan")
        dout[poison_row] = float("nan")
        if h0 is not None:
            h0[:, poison_row] = float("nan")
    whh = torch.from_numpy(np.array(c.whh)).cuda()
    bhh = None if c.bhh is None else torch.from_numpy(np.array(c.bhh)).cuda()
    return gi, whh, bhh, h0, dout


def _result(c, out, sav, dgi, dgh, dh0):
    """Standard-layout numpy outputs (for bitwise comparisons) and the processing-order dict of errors()."""
    nd, H = c.nd, c.H
    raw = {"out": out, "sav": sav, "dgi": dgi, "dgh": dgh, "dh0": dh0}
    got = {"h": proc(out, nd, 1)[:, :, :, 0], "sav": proc(sav, nd, 4), "dgi": proc(dgi, nd, 3),
           "dgh": proc(dgh, nd, 3), "dh0": dh0}
    return raw, got


def run_gru16(c, poison_row=None):
    """b2p_gru_lane_permute -> b2p_gru_fwd16 / b2p_gru_bwd16 -> b2p_gru_lane_permute with the rmaps of
    functional.py; saved is unpacked on the host by ln_permute (functional.py never unpacks it)."""
    import torch
    lib = _lib()
    B, T, H, nd = c.B, c.T, c.H, c.nd
    gi, whh, bhh, h0, dout = _device_inputs(c, "gru16", poison_row)
    p = lambda t: None if t is None else t.data_ptr()
    st = lib.stream_ptr()
    lnf = lambda R: int(lib.load().b2p_gru16_lane_floats(B, T, H, nd, R))
    assert lnf(3) == ln_floats(B, T, H, nd, 3)
    g = Guarded()
    giL, hL, savL, doL, dgL = g.new(lnf(3)), g.new(lnf(1)), g.new(lnf(4)), g.new(lnf(1)), g.new(lnf(4))
    out, dgi, dgh = g.new(B * T * nd * H), g.new(B * T * nd * 3 * H), g.new(B * T * nd * 3 * H)
    dh0 = g.new(nd * B * H) if h0 is not None else None
    lib.call("b2p_gru_lane_permute", p(gi), p(giL), B, T, H, nd, 3, 3, 0x210, 1, st)
    lib.call("b2p_gru_fwd16", p(giL), p(whh), p(bhh), p(h0), p(hL), p(savL), B, T, H, nd, st)
    lib.call("b2p_gru_lane_permute", p(hL), p(out), B, T, H, nd, 1, 1, 0x0, 0, st)
    lib.call("b2p_gru_lane_permute", p(dout), p(doL), B, T, H, nd, 1, 1, 0x0, 1, st)
    lib.call("b2p_gru_bwd16", p(doL), p(whh), p(hL), p(savL), p(h0), p(dgL), p(dh0), B, T, H, nd, st)
    lib.call("b2p_gru_lane_permute", p(dgL), p(dgi), B, T, H, nd, 4, 3, 0xF210, 0, st)
    lib.call("b2p_gru_lane_permute", p(dgL), p(dgh), B, T, H, nd, 4, 3, 0x2F10, 0, st)
    torch.cuda.synchronize()
    g.check(finite=poison_row is None)
    sav = ln_permute(savL.cpu().numpy(), np.zeros(B * T * nd * 4 * H, F32), B, T, H, nd, 4, 4, 0x3210, 0)
    n = lambda t, *s: t.cpu().numpy().reshape(*s)
    return _result(c, n(out, B, T, nd * H), sav.reshape(B, T, nd * 4 * H), n(dgi, B, T, nd * 3 * H),
                   n(dgh, B, T, nd * 3 * H), None if dh0 is None else n(dh0, nd, B, H))


def run_mc(c, poison_row=None):
    """b2p_gru_fwd_mc / b2p_gru_bwd_mc with b2p_gru_mc_workspace; the fail word must be 0 after each pass."""
    import torch
    lib = _lib()
    B, T, H, nd = c.B, c.T, c.H, c.nd
    gi, whh, bhh, h0, dout = _device_inputs(c, "mc", poison_row)
    p = lambda t: None if t is None else t.data_ptr()
    st = lib.stream_ptr()
    g = Guarded()
    out, sav = g.new(B * T * nd * H), g.new(B * T * nd * 4 * H)
    dgi, dgh = g.new(B * T * nd * 3 * H), g.new(B * T * nd * 3 * H)
    dh0 = g.new(nd * B * H) if h0 is not None else None
    ws = torch.empty(int(lib.load().b2p_gru_mc_workspace(B, H, nd)), device="cuda", dtype=torch.uint8)
    lib.call("b2p_gru_fwd_mc", p(gi), p(whh), p(bhh), p(h0), p(out), p(sav), p(ws), B, T, H, nd, st)
    f1 = ws[:4].clone()
    lib.call("b2p_gru_bwd_mc", p(dout), p(whh), p(out), p(sav), p(h0), p(dgi), p(dgh), p(dh0), p(ws), B, T, H, nd, st)
    torch.cuda.synchronize()
    assert int(f1.abs().sum()) == 0 and int(ws[:4].abs().sum()) == 0, f"H={H}: a member timed out"
    g.check(finite=poison_row is None)
    n = lambda t, *s: t.cpu().numpy().reshape(*s)
    return _result(c, n(out, B, T, nd * H), n(sav, B, T, nd * 4 * H), n(dgi, B, T, nd * 3 * H),
                   n(dgh, B, T, nd * 3 * H), None if dh0 is None else n(dh0, nd, B, H))


RUNNERS = {"gru16": run_gru16, "mc": run_mc}
