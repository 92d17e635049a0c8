"""What tests/test_attn16_edges_gpu.py and tests/test_attn16_bound_host.py share for the fused 16-bit attention of
csrc/attn16.hip: the lengths, the inputs with their planted spikes, the numpy restatement of the dropout hash, the
float64 restatement of the operation, the per-element bound, and the runs of the C entry points.

Shapes. B = 2, two heads of 64 (batch and head strides both exercised), T' on the edges of the 16-row tiles, the
128-row blocks and the three shape classes (T' <= 240, the T1 forms of 241..256, the 512-key class of 257..512).

Inputs. A generator seeded by T' draws qkv = randn * 0.7 and dO = randn; both are rounded to bf16 (and qkv then to
fp16 for the fp16 entry points). Every reference upcasts the 16-bit tensors the kernel is handed, so the rounding of
the inputs is not part of any error. Spikes: for each edge key e in {0, 15, 16, 127, 128, 255, 256, 383, 384, T'-1},
e < T', and each (batch, head) a random +-1 vector r: k[e] = r, v[e] = 3 r, and q = r + 0.1 randn for the queries e
and (7e + 3) mod T'. The spiked score is 8 (softmax weight about 0.8 to 0.99), so a key that is left out or taken
twice moves single rows of O and of the gradients by far more than any rounding. (Amplitude 2 would give a score of
32: 1 - P then cancels in float64 itself and the restatement stops being a reference.)

Reference (ref64). softmax(Q K^T scale) -> keep / (1 - p) -> @ V and its gradients in float64 on the CPU, with every
intermediate the bound needs: z = scores in the log2 domain, lse2, P, P_d = P keep / (1 - p), dP = dO V^T, delta =
sum_key P_d dP, dS = P (dP keep / (1 - p) - delta). p is the float32 value the kernel receives. The keep mask is
keep_mask_ref, a numpy restatement of b2p_keep (csrc/common.h), under the seed of seed_eff, a restatement of
b2p_seed_eff: never what a kernel or the unfused path drew.

The rule (bounds). Every output element obeys |kernel - ref64| <= bound, the bound being the first-order worst-case
propagation of each rounding on that element's path, computed in float64 from absolute values. No factor is fitted.
Unit roundoffs: bf16 U_BF = 2^-8, fp16 U_HF = 2^-11, fp32 U = 2^-24. UA = 2^-23 is charged per addition of an MFMA
accumulation (the matrix unit's accumulator is not documented to round to nearest: a whole ulp) and per hardware
exp2 / log2 (one ulp). TM = 256 or 512 is the key capacity of the shape class, H the fp16 mode.

  fp32 terms (one formula each, from the loop named):
    dz     = 64 UA c2 (|Q| @ |K|^T) + 4 U (|z| + |zmax|)       scores: two chained 32-wide MFMAs = 64 products per
                                                                score; c2 = scale * log2(e) (its product and the
                                                                scale's own rounding), m * c2, the exponent's fma
    rho_e  = ln2 dz + UA                                        exp2 of a perturbed argument, one ulp of v_exp_f32
    n_sum  = TM / 4 + 2                                         row sum: TM / 16 tiles x 4 registers per lane, then two
                                                                cross-lane shuffles
    rho_s  = max_key rho_e + n_sum U                            the row sum, relative
    rho_P  = rho_e + rho_s + 5 U                                forward P_d: 1 / sum, times 1 / (1 - p) (itself 1 - p
                                                                and a division on the host), times e
    b_lse2 = rho_s / ln2 + UA |lse2 - zmax| + U |lse2| + 2 U |zmax|
                                                                log2(sum) of a perturbed sum, one ulp of v_log_f32,
                                                                the final addition, m * c2 against the exact c2
    rho_B  = ln2 (dz + b_lse2 + U |z - lse2|) + UA              backward P = exp2(z - lse2) from the stored lse2
    d_dP   = 64 UA (|dO| @ |V|^T)  [+ |dO| @ res(V)^T, H]       dP: 64 products; H: V rounded fp16 -> bf16 (to_b16),
                                                                res(x) = |x - bf16(x)| <= U_BF |x|: the rounding of
                                                                an operand is known from the input, so the residual
                                                                itself is propagated and not its worst case
    d_PD   = d_dP ks + 3 U |dP| ks,  ks = keep / (1 - p)        dP * keep scale
    b_delta = sum_key (P d_PD + rho_B P |dP| ks) + (n_sum + 1) U sum_key P |dP| ks
                                                                delta = sum_key P (dP ks): the product, the lane's
                                                                TM / 4 additions and two shuffles
    d_dS   = P (d_PD + b_delta + U (|dP| ks + |delta|)) + (rho_B + U) |dS|
                                                                dS = P (dP ks - delta): the cancellation in the
                                                                difference carries the absolute errors of both sides
    every MFMA product over the keys or queries: T' UA (sum of absolute terms); the store's multiplication by scale and
    the scale's own rounding: 2 U |dQ|, 2 U |dK|.

  16-bit terms, per output:
    O      u_p (P_d @ |V|)            P_d rounded to the operand type before P_d V (u_p = U_BF, H: U_HF)
           2^-25 sum_key |V|   (H)    fp16 P_d below 2^-14 is subnormal: absolute 2^-25 per key
           u_o |O|  [+ 2^-25, H]      O rounded on store (fp16 in H, subnormal below 2^-14); the bf16 copy Ob16 of the
                                      fp16 forward is rounded from the fp32 accumulator: U_BF |O|
           + ((rho_P P_d) @ |V|) + T' UA (P_d @ |V|)
    dV     U_BF (P_d^T @ |dO|)        P_d rounded to bf16 in both modes
           + (((rho_B + 3 U) P_d)^T @ |dO|) + T' UA (P_d^T @ |dO|)
    dK     scale [U_BF (|dS|^T @ |Q|) dS rounded to bf16 in both modes
           + (|dS|^T @ res(Q)), H     Q rounded fp16 -> bf16 (to_b16)
           + (d_dS^T @ |Q|) + T' UA (|dS|^T @ |Q|)] + 2 U |dK|
    dQ     scale [u_s (|dS| @ |K|)    dS rounded to bf16 (bf16 mode, and H in the 512-key class); H at T' <= 256: the row
                                      is scaled by the power of two 2^-em that puts its largest |dS| in [1, 2) and
                                      rounded to fp16: u_s = U_HF
           + 2^-25 rowmax(|dS| + d_dS) sum_key |K|, H at T' <= 256: scaled values below 2^-14 are subnormal, absolute
                                      2^-25 2^em, and 2^em is at most the largest |dS| the kernel holds
           + (|dS| @ res(K)), H in the 512-key class: K rounded fp16 -> bf16 (to_b16)
           + (d_dS @ |K|) + T' UA (|dS| @ |K|)] + 2 U |dQ|
    dqkv16 the fp32 image's bound + U_BF |ref|
    lse2   b_lse2; delta: b_delta. Both are fp32 outputs: fp32 terms alone (H: delta carries d_dP's V term).
"""
import ctypes
import functools
import math
import types

import numpy as np
import torch

B, NH, DH = 2, 2, 64
D = NH * DH
SCALE = DH ** -0.5
LOG2E = 1.0 / math.log(2.0)
LN2 = math.log(2.0)
U_BF, U_HF, U, UA = 2.0 ** -8, 2.0 ** -11, 2.0 ** -24, 2.0 ** -23
SUB_HF = 2.0 ** -25                    # half the spacing of the fp16 subnormals
P_DROP = float(np.float32(0.1))        # the float32 value the entry points receive
SEED = 0x1234567890ABCDEF             # both 32-bit halves of the seed reach the hash key
EPOCH = 7                              # the device step counter of the epoch cases

T_256 = (1, 2, 3, 15, 16, 17, 127, 128, 129, 240, 241, 255, 256)
T_512 = (257, 383, 384, 385, 496, 497, 511, 512)
T_ALL = T_256 + T_512
T_EPOCH = (17, 249, 313)               # one T' per shape class
EDGE_KEYS = (0, 15, 16, 127, 128, 255, 256, 383, 384)


def forms(T):
    """The dropout forms the entry points accept at T': (name, p)."""
    out = [("none", 0.0), ("hash", P_DROP)]
    if T <= 256:
        out += [("stored", P_DROP), ("ahead", P_DROP)]
    return out


# ------------------------------------------------------------------------------------------- dropout hash
def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def keep_mask_ref(seed, p, B, nh, T):
    """numpy restatement of the dropout keep mask (csrc/common.h b2p_keep over the attention element
    index ((b*nh + h)*T + q)*TP + key, TP = T rounded up to even): (B, nh, T, T) bool."""
    with np.errstate(over="ignore"):
        k = np.uint32(seed & 0xFFFFFFFF) ^ _mix32(np.uint32(((seed >> 32) + 0x9E3779B9) & 0xFFFFFFFF))
        TP = T + (T & 1)
        row = np.arange(B * nh * T, dtype=np.uint64)[:, None] * np.uint64(TP)
        idx = (row + np.arange(T, dtype=np.uint64)[None, :]).astype(np.uint32)
        h = _mix32(_mix32((idx >> np.uint32(1)) ^ k) + k)
        half = np.where(idx & np.uint32(1), h >> np.uint32(16), h & np.uint32(0xFFFF))
    thr = int(float(np.float32(p)) * 4294967296.0)   # b2p_dropout_threshold of the float32 p
    thr16 = (thr >> 16) + ((thr >> 15) & 1)
    return (half >= thr16).reshape(B, nh, T, T)


def seed_eff(seed, epoch=None):
    """Restatement of b2p_seed_eff (csrc/common.h): the seed a launch hashes with under a device step counter
    holding `epoch` (None: no counter set), in 64-bit wrapping arithmetic."""
    if epoch is None:
        return int(seed)
    with np.errstate(over="ignore"):
        return int(np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * np.uint64(epoch))


def decode_mask_words(words, T):
    """(B, nh, T, 8) int32 keep words (the layout the storing forward and b2p_attn16_keep_masks write: byte 8g + c,
    g = (key >> 2) & 3, c = key >> 5) -> (B, nh, T, T) bool."""
    w32 = words.cpu().numpy().view(np.uint32)
    keys = np.arange(256)
    w = (keys >> 7) + 2 * ((keys >> 2) & 3)
    sh = (8 * ((keys >> 5) & 3) + 4 * ((keys >> 4) & 1) + (keys & 3)).astype(np.uint32)
    return (((w32[..., w] >> sh) & 1)[..., :T]).astype(bool)


@functools.lru_cache(maxsize=4)
def keep_ref(T, epoch=None):
    return torch.from_numpy(keep_mask_ref(seed_eff(SEED, epoch), P_DROP, B, NH, T))


# ------------------------------------------------------------------------------------------------- inputs
def heads(x, T):   # (B*T, nh*dh) -> (B, nh, T, dh)
    return x.view(B, T, NH, DH).permute(0, 2, 1, 3)


def rows(x, T):    # (B, nh, T, dh) -> (B*T, nh*dh)
    return x.permute(0, 2, 1, 3).reshape(B * T, D)


@functools.lru_cache(maxsize=None)
def inputs(T, spikes=True, qkv_dtype=torch.bfloat16):
    """qkv (B*T, 3D) rounded to qkv_dtype and dO (B*T, D) in bf16."""
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B * T, 3 * D, generator=g) * 0.7
    dO = torch.randn(B * T, D, generator=g)
    if spikes:
        q, k, v = (qkv[:, i * D:(i + 1) * D].view(B, T, NH, DH) for i in range(3))
        for e in sorted({e for e in EDGE_KEYS + (T - 1,) if e < T}):
            r = torch.where(torch.randn(B, NH, DH, generator=g) < 0, -1.0, 1.0)
            k[:, e] = r
            v[:, e] = 3 * r
            for qi in (e, (7 * e + 3) % T):
                q[:, qi] = r + 0.1 * torch.randn(B, NH, DH, generator=g)
    return qkv.to(qkv_dtype), dO.to(torch.bfloat16)


def operands(T, half, spikes=True, via_bf16=True):
    """The 16-bit tensors handed to the kernel: qkv in fp16 (half) or bf16, dO in bf16. via_bf16 False (half only):
    qkv rounded to fp16 directly, so its values are not bf16 numbers and to_b16 in the backward does round."""
    if half and not via_bf16:
        return inputs(T, spikes, torch.float16)
    qkv, dO = inputs(T, spikes)
    return (qkv.to(torch.float16) if half else qkv), dO


# ------------------------------------------------------------------------------------- float64 restatement
def ref64(qkv16, dO16, T, keep=None, p=0.0):
    """The operation in float64 from the 16-bit operands; keep (B, nh, T, T) bool or None. Row-major outputs O
    (B*T, D), dqkv (B*T, 3D); lse2, delta (B, nh, T); and the (B, nh, T, .) intermediates of the bound."""
    x = qkv16.double()
    q, k, v = (heads(x[:, i * D:(i + 1) * D], T) for i in range(3))
    dOh = heads(dO16.double(), T)
    S = q @ k.transpose(-1, -2) * SCALE
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    ks = torch.ones_like(P) if keep is None else keep.double() / (1.0 - p)
    Pd = P * ks
    Oh = Pd @ v
    dP = dOh @ v.transpose(-1, -2)
    delta = (Pd * dP).sum(-1)
    dS = P * (dP * ks - delta[..., None])
    dQ, dK, dV = dS @ k * SCALE, dS.transpose(-1, -2) @ q * SCALE, Pd.transpose(-1, -2) @ dOh
    z = S * LOG2E
    return types.SimpleNamespace(
        T=T, q=q, k=k, v=v, dOh=dOh, z=z, zmax=z.amax(-1), lse2=lse * LOG2E, P=P, ks=ks, Pd=Pd, dP=dP, delta=delta,
        dS=dS, Oh=Oh, dQ=dQ, dK=dK, dV=dV, O=rows(Oh, T), dqkv=torch.cat([rows(dQ, T), rows(dK, T), rows(dV, T)], 1))


def _res_bf16(x):
    """|x - bf16(x)|: what to_b16 does to an fp16 operand is a function of the input alone, so the residual itself
    (at most U_BF |x|) is propagated, not its worst case."""
    return (x - x.to(torch.float32).to(torch.bfloat16).double()).abs()


def bounds(r, half):
    """The per-element bounds of the module docstring for the reference r: a dict of float64 tensors shaped like
    the outputs: O, Ob (the fp16 forward's bf16 copy; bf16 mode: O itself), lse2, delta, dqkv, dqkv16."""
    T = r.T
    long = T > 256
    TM = 512 if long else 256
    t = lambda x: x.transpose(-1, -2)
    aq, ak, av, ado = r.q.abs(), r.k.abs(), r.v.abs(), r.dOh.abs()
    c2 = SCALE * LOG2E
    # fp32 terms
    dz = 64 * UA * c2 * (aq @ t(ak)) + 4 * U * (r.z.abs() + r.zmax.abs()[..., None])
    rho_e = LN2 * dz + UA
    n_sum = TM // 4 + 2
    rho_s = rho_e.amax(-1) + n_sum * U
    rho_P = rho_e + rho_s[..., None] + 5 * U
    b_lse2 = rho_s / LN2 + UA * (r.lse2 - r.zmax).abs() + U * r.lse2.abs() + 2 * U * r.zmax.abs()
    rho_B = LN2 * (dz + b_lse2[..., None] + U * (r.z - r.lse2[..., None]).abs()) + UA
    d_dP = 64 * UA * (ado @ t(av)) + (ado @ t(_res_bf16(r.v)) if half else 0.0)
    aPD = r.dP.abs() * r.ks
    d_PD = d_dP * r.ks + 3 * U * aPD
    b_delta = (r.P * d_PD + rho_B * r.P * aPD).sum(-1) + (n_sum + 1) * U * (r.P * aPD).sum(-1)
    adS = r.dS.abs()
    d_dS = r.P * (d_PD + b_delta[..., None] + U * (aPD + r.delta.abs()[..., None])) + (rho_B + U) * adS
    # O
    u_p = U_HF if half else U_BF
    PV = r.Pd @ av
    core = u_p * PV + (rho_P * r.Pd) @ av + T * UA * PV
    if half:
        core = core + SUB_HF * av.sum(-2, keepdim=True)
    aO = r.Oh.abs()
    b_O = core + ((U_HF * aO + SUB_HF) if half else U_BF * aO)
    b_Ob = core + U_BF * aO
    # dV
    PtdO = t(r.Pd) @ ado
    b_dV = U_BF * PtdO + t((rho_B + 3 * U) * r.Pd) @ ado + T * UA * PtdO
    # dK
    SQ = t(adS) @ aq
    b_dK = SCALE * (U_BF * SQ + (t(adS) @ _res_bf16(r.q) if half else 0.0) + t(d_dS) @ aq + T * UA * SQ) \
        + 2 * U * r.dK.abs()
    # dQ
    SK = adS @ ak
    if half and not long:
        sixteen = U_HF * SK + SUB_HF * (adS + d_dS).amax(-1, keepdim=True) * ak.sum(-2, keepdim=True)
    else:
        sixteen = U_BF * SK + (adS @ _res_bf16(r.k) if half else 0.0)
    b_dQ = SCALE * (sixteen + d_dS @ ak + T * UA * SK) + 2 * U * r.dQ.abs()
    b_dqkv = torch.cat([rows(b_dQ, T), rows(b_dK, T), rows(b_dV, T)], 1)
    return {"O": rows(b_O, T), "Ob": rows(b_Ob, T), "lse2": b_lse2, "delta": b_delta, "dqkv": b_dqkv,
            "dqkv16": b_dqkv + U_BF * r.dqkv.abs()}


def references(r):
    """The reference value of every bounded output, keyed like bounds()."""
    return {"O": r.O, "Ob": r.O, "lse2": r.lse2, "delta": r.delta, "dqkv": r.dqkv, "dqkv16": r.dqkv}


def worst_ratios(got, r, bnd):
    """max |got - ref| / bound per output (inf where an element is not finite or a zero bound is missed)."""
    ref = references(r)
    out = {}
    for name, x in got.items():
        err = (x.detach().double().cpu() - ref[name]).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd[name])
        ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
        out[name] = float(ratio.max())
    return out


# -------------------------------------------------------------------------------------------------- GPU runs
def fn():
    from wav2vec2forbrain_amd import functional as Fn
    return Fn


SENTINEL = 0x5A5A5A5A    # the fill of the keep-word allocation (int32 holds no NaN)


def guarded(shape, dtype, guard):
    """A contiguous `shape` view into a larger allocation with `guard` elements in front and behind, all filled
    with NaN (the keep words: SENTINEL). guard is a multiple of 16 bytes, so the view stays 16-byte aligned."""
    n = int(np.prod(shape))
    assert (guard * torch.empty((), dtype=dtype).element_size()) % 16 == 0
    fill = SENTINEL if dtype == torch.int32 else float("nan")
    whole = torch.full((n + 2 * guard,), fill, dtype=dtype, device="cuda")
    view = whole[guard:guard + n].view(shape)
    assert view.data_ptr() % 16 == 0
    return view, whole, guard


class Bufs:
    """Every output of one forward + backward as a view between guard rows: one row's worth in front and behind
    (lse2 / delta: T' floats rounded up to 16 bytes)."""

    def __init__(self, T, half, mask):
        g1 = -(-T // 4) * 4
        self.T, self.half = T, half
        self.g = {"O": guarded((B * T, D), torch.float16 if half else torch.bfloat16, D),
                  "lse2": guarded((B, NH, T), torch.float32, g1),
                  "delta": guarded((B, NH, T), torch.float32, g1),
                  "dqkv": guarded((B * T, 3 * D), torch.float32, 3 * D),
                  "dqkv16": guarded((B * T, 3 * D), torch.bfloat16, 3 * D)}
        if half:
            self.g["Ob"] = guarded((B * T, D), torch.bfloat16, D)
        if mask:
            self.g["mask"] = guarded((B, NH, T, 8), torch.int32, 8)

    def __getitem__(self, name):
        return self.g[name][0]

    def outputs(self):
        return {k: v[0] for k, v in self.g.items() if k != "mask"}

    def check(self, nb=B):
        """Guards untouched; every element of the first nb batches finite (written, nothing left of the fill)."""
        for name, (view, whole, guard) in self.g.items():
            front, back = whole[:guard], whole[guard + view.numel():]
            if name == "mask":
                assert bool((front == SENTINEL).all()) and bool((back == SENTINEL).all()), name
                continue
            assert bool(torch.isnan(front).all()) and bool(torch.isnan(back).all()), (name, self.T)
            assert bool(torch.isfinite(view[:view.shape[0] * nb // B]).all()), (name, self.T)


def run(T, half, form, p, qkv=None, dO=None, dkv=1, fwd=True, bufs=None):
    """One forward (unless fwd is False: bufs then holds a forward's lse2 and keep words) and one backward through
    the C entry points into guarded buffers. form: none / hash (the backward rehashes) / stored (the forward
    stores the keep bits, the backward reads them) / ahead (b2p_attn16_keep_masks draws them, b2p_attn16_fwd*_keep
    and the backward read them). dkv: the dK/dV kernel form (b2p_attn16_dkv_variant)."""
    Fn = fn()
    lib = Fn._lib.load()
    if qkv is None:
        qkv, dO = (x.cuda() for x in operands(T, half))
    masked = form in ("stored", "ahead")
    if bufs is None:
        bufs = Bufs(T, half, masked)
    mp = bufs["mask"].data_ptr() if masked else None
    st, pf, sc = Fn._st(), float(p), float(SCALE)
    if fwd:
        o2 = (bufs["O"].data_ptr(), bufs["Ob"].data_ptr()) if half else (bufs["O"].data_ptr(),)
        if form == "ahead":
            seeds = (ctypes.c_uint64 * 1)(SEED)
            Fn._lib.call("b2p_attn16_keep_masks", mp, ctypes.addressof(seeds), 1, B, T, NH, pf, st)
            Fn._lib.call("b2p_attn16_fwd_f16_keep" if half else "b2p_attn16_fwd_keep", qkv.data_ptr(), *o2,
                         bufs["lse2"].data_ptr(), B, T, NH, DH, sc, pf, mp, st)
        else:
            Fn._lib.call("b2p_attn16_fwd_f16" if half else "b2p_attn16_fwd", qkv.data_ptr(), *o2,
                         bufs["lse2"].data_ptr(), B, T, NH, DH, sc, pf, SEED, mp, st)
    try:
        Fn._lib.check(lib.b2p_attn16_dkv_variant(dkv), "dkv_variant")
        Fn._lib.call("b2p_attn16_bwd_f16" if half else "b2p_attn16_bwd", qkv.data_ptr(), dO.data_ptr(),
                     bufs["lse2"].data_ptr(), bufs["delta"].data_ptr(), bufs["dqkv"].data_ptr(),
                     bufs["dqkv16"].data_ptr(), B, T, NH, DH, sc, pf, SEED, mp, st)
        torch.cuda.synchronize()
    finally:
        Fn._lib.check(lib.b2p_attn16_dkv_variant(1), "dkv_variant")
    return bufs


def bits(x):
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


def bound_case(T, half, epoch=None, form_list=None, via_bf16=True):
    """Every dropout form of T' in one operand type against float64 under the per-element bound, with the guard
    rows, the agreement of the two dK/dV kernels and the decode of the keep words. Prints and returns the worst
    |err| / bound per output over the forms."""
    qkv16, dO16 = operands(T, half, via_bf16=via_bf16)
    qkv, dO = qkv16.cuda(), dO16.cuda()
    worst, fails = {}, []
    refs = {}
    for form, p in (form_list or forms(T)):
        keep = keep_ref(T, epoch) if p > 0 else None
        if p not in refs:
            r = ref64(qkv16, dO16, T, keep, p)
            refs[p] = (r, bounds(r, half))
        r, bnd = refs[p]
        bufs = run(T, half, form, p, qkv, dO)
        bufs.check()
        got = {k: v.clone() for k, v in bufs.outputs().items()}
        if "mask" in bufs.g:
            assert np.array_equal(decode_mask_words(bufs["mask"], T), keep.numpy()), (T, form)
        run(T, half, form, p, qkv, dO, dkv=0, fwd=False, bufs=bufs)     # the per-tile dK/dV kernel: bitwise equal
        bufs.check()
        for name in ("dqkv", "dqkv16", "delta"):
            assert torch.equal(bits(got[name]), bits(bufs[name])), (T, form, name)
        ratios = worst_ratios(got, r, bnd)
        for name, x in ratios.items():
            worst[name] = max(worst.get(name, 0.0), x)
            if not x <= 1.0:
                fails.append((form, name, x))
    tag = f"attn16 {'fp16' if half else 'bf16'} T'={T}" + ("" if epoch is None else f" epoch={epoch}") \
        + ("" if via_bf16 else " fp16-only qkv")
    print(tag + " worst |err|/bound: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst, fails
