"""16-bit output images (pre16, C16, C16b) and the aux16 read of the register epilogue of the 16-bit-operand
GEMM kernels: every image must hold exactly the bits of the fp32 result of the same GEMM rounded to the
image's format, whatever store / load width a launch takes (16 B per lane where base, leading dimension,
batch strides and N allow it, 8 B otherwise), and nothing outside [0, M) x [0, N) may be written.

The fp32 stores (C, 16 B per lane from the accumulator layout) are the independent reference: the same GEMM
is run again with only an fp32 C (same bias, activation, dropout seed, aux16) for the final value, and with
only the bias for the pre-activation.

Shapes are the smallest at which the paired-column-tile store can go wrong: M in {1, 200, 391} (a partial
32-row band, a partial row tile, a partial 192 / 256-row tile spanning two workgroups), N in {8, 264, 520}
(one 8-column group, a partial 64-column wave tile, two 256-column tiles with a partial one), N in {68, 260}
(N % 8 != 0: the 8-byte form), N = 2056 (past the narrow kernels' limit: the 128 x 128 kernel in the `small`
family), a C16 base 8-byte but not 16-byte aligned, ldc > N inside a wider tensor, and a batched launch.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

# kernel family, forced by environment (read once per process: one child process per family)
_ENV = {"small": {"B2P_GEMM16_PP": "0"},
        "pp": {"B2P_GEMM16_PP": "2", "B2P_GEMM16_PP192": "0"},
        "pp192": {"B2P_GEMM16_PP": "2", "B2P_GEMM16_PP192": "2"}}

SENT = 0x7FA5          # a NaN pattern in bf16 and in fp16: no finite result has these bits
SENT32 = 0x7FA5A5A5    # the same for fp32
K = 64
SEED = 1234
DROP = 0.1

_SHAPES = [(M, N) for M in (1, 200, 391) for N in (8, 264, 520)] + [(200, 260), (200, 68), (200, 2056)]
_KINDS = ("BADHHB", "BADH", "GDH16CS")


def _fn():
    from wav2vec2forbrain_amd import functional as Fn
    return Fn


class _Img:
    """An M x N 16-bit image (per batch member) inside a sentinel-filled buffer with a guard row:
    lay "plain" (contiguous), "off4" (base offset by 4 elements: 8-byte, not 16-byte aligned), "slice" (columns
    8 .. 8 + N of rows N + 24 wide)."""

    def __init__(self, M, N, dtype, lay="plain", nz=1):
        self.M, self.N, self.nz = M, N, nz
        rows = nz * M
        if lay == "slice":
            assert nz == 1
            self.ld = N + 24
            self.buf = torch.empty((rows + 1) * self.ld, device="cuda", dtype=dtype)
            self.off = 8
        else:
            self.ld = N
            self.off = 4 if lay == "off4" else 0
            self.buf = torch.empty((rows + 1) * N + 8, device="cuda", dtype=dtype)
        self.buf.view(torch.int16).fill_(SENT)
        # the launch's view: base at the image's first element (functional._p adds no further offset)
        self.t = self.buf[self.off:]
        n = rows * self.ld
        self.mask = torch.zeros(self.buf.numel(), device="cuda", dtype=torch.bool)
        m = self.mask[self.off:self.off + n].view(rows, self.ld)
        m[:, :N] = True

    def get(self):
        rows = self.nz * self.M
        return self.buf[self.off:self.off + rows * self.ld].view(rows, self.ld)[:, :self.N]

    def check(self, want, what):
        bits = self.buf.view(torch.int16)
        assert bool((bits[~self.mask] == SENT).all()), f"{what}: written outside the image"
        assert not bool((bits[self.mask] == SENT).any()), f"{what}: elements left unwritten"
        got = self.get()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
            f"{what}: {int((got.view(torch.int16) != want.view(torch.int16)).sum())} elements differ"


def _operands(Fn, M, N, dt, nz):
    a = torch.randn(nz * M, K, device="cuda").to(dt)
    w = torch.randn(N, K, device="cuda").to(dt)
    A = Fn.op(a, 0, K, True, bs1=M * K if nz > 1 else 0)
    B = Fn.op(w, 0, K, True)
    return (a, w), A, B


def _f32(rows, N):
    """fp32 reference output with a guard row, sentinel-filled."""
    t = torch.empty(rows + 1, N, device="cuda")
    t.view(torch.int32).fill_(SENT32)
    return t


def _check_f32(t, rows, what):
    assert bool((t[rows:].view(torch.int32) == SENT32).all()), f"{what}: guard row written"
    assert not bool((t[:rows].view(torch.int32) == SENT32).any()), f"{what}: elements left unwritten"
    return t[:rows]


def _check_case(kind, M, N, lay="plain", nz=1):
    Fn = _fn()
    torch.manual_seed(11)
    what = f"{kind} {M}x{N} {lay} nz={nz}"
    rows = nz * M
    bz = dict(nz1=nz, cbs1=M * N) if nz > 1 else {}
    bf = torch.bfloat16
    if kind in ("BADHHB", "BADH"):
        h = kind == "BADHHB"                      # fp16 operands, fp16 C16 and a second bf16 copy
        dt = torch.float16 if h else bf
        keep, A, B = _operands(Fn, M, N, dt, nz)
        bias = torch.randn(N, device="cuda")
        pre16 = _Img(M, N, bf, "slice" if lay == "slice" else "plain", nz)
        c16 = _Img(M, N, dt, lay, nz)
        kw = dict(bias=bias, act=Fn.ACT["gelu"], drop_p=DROP, seed=SEED)
        img = dict(pre16=pre16.t, C16=c16.t, c16_fp16=h)
        c16b = None
        if h:
            c16b = _Img(M, N, bf, "slice" if lay == "slice" else "plain", nz)
            img["C16b"] = c16b.t
        Fn.gemm(M, N, K, A, B, None, c16.ld, **bz, **kw, **img)
        C, P = _f32(rows, N), _f32(rows, N)
        Fn.gemm(M, N, K, A, B, C, N, **bz, **kw)
        Fn.gemm(M, N, K, A, B, P, N, **bz, bias=bias)
        torch.cuda.synchronize()
        C, P = _check_f32(C, rows, what + " C"), _check_f32(P, rows, what + " pre")
        pre16.check(P.to(bf), what + " pre16")
        c16.check(C.to(dt), what + " C16")
        if c16b is not None:
            c16b.check(C.to(bf), what + " C16b")
        # the dropout must have been on (and identical in both launches): some exact zeros, not all
        z = float((C == 0).float().mean())
        assert M * N < 64 or 0.0 < z < 0.5, f"{what}: dropped fraction {z}"
    else:                                         # backward-data: dropout, GELU' on aux16, bf16 C16, column sums
        keep, A, B = _operands(Fn, M, N, bf, nz)
        aux = _Img(M, N, bf, "slice" if lay == "slice" else "plain", nz)
        aux.get().copy_(torch.randn(rows, N, device="cuda").to(bf))
        c16 = _Img(M, N, bf, lay, nz)
        assert aux.ld == c16.ld
        kw = dict(act_bwd=Fn.ACT["gelu"], drop_p=DROP, seed=SEED)
        parts = Fn.colsum_parts_buf(M, N, "cuda") if nz == 1 else None
        Fn.gemm(M, N, K, A, B, None, c16.ld, **bz, **kw, aux16=aux.t, C16=c16.t, colsum_part=parts)
        C = _f32(rows, N)
        auxc = aux.get().contiguous()
        Fn.gemm(M, N, K, A, B, C, N, **bz, **kw, aux16=auxc)
        torch.cuda.synchronize()
        C = _check_f32(C, rows, what + " C")
        c16.check(C.to(bf), what + " C16")
        aux.check(auxc, what + " aux16 (read only)")
        if parts is not None:
            cs = Fn.colsum_from_parts(parts, torch.empty(N, device="cuda"))
            err, scale = float((cs - C.sum(0)).abs().max()), float(C.abs().sum(0).max())
            assert err <= 1e-3 * scale + 1e-4, f"{what}: column sums off by {err} (scale {scale})"
    del keep


def _run_all():
    for kind in _KINDS:
        for M, N in _SHAPES:
            _check_case(kind, M, N)
        _check_case(kind, 200, 264, lay="off4")     # 8-byte aligned C16 base: the 8-byte form, still exact
        _check_case(kind, 200, 264, lay="slice")    # ldc = N + 24 > N: columns outside the slice untouched
        _check_case(kind, 391, 520, lay="slice")
        _check_case(kind, 200, 264, nz=3)           # batched, cbs1 = M * N
        _check_case(kind, 391, 520, nz=3)


@pytest.mark.parametrize("family", ["small", "pp", "pp192"])
def test_16bit_images_bitwise(family):
    """pre16 / C16 / C16b of K_BADHHB (fp16 operands) and K_BADH (bf16), C16 and the fused column sums of
    K_GDH16CS, bitwise against the fp32-output launch of the same GEMM, in each kernel family."""
    env = dict(os.environ, **_ENV[family])
    code = "import tests.test_gemm_epilogue_wide_gpu as t\nt._run_all()\n"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
