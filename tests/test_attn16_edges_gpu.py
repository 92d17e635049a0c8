"""The fused 16-bit attention (csrc/attn16.hip: b2p_attn16_fwd / _bwd, their fp16 forms, the storing forward,
b2p_attn16_keep_masks with b2p_attn16_fwd*_keep, both dK/dV kernels) against a float64 restatement, element by
element, at the edges of its tiles, blocks and shape classes. tests/attn16_cases.py holds the cases, the restatement
and the derivation of the bound (every rounding counted and the formula of each term); tests/test_attn16_bound_host.py
shows on the host that the bound accepts a correctly rounded computation and rejects one with a key dropped in the last
tile, a keep bit inverted or the last tile's scores off by 5 %.

T' in {1, 2, 3, 15, 16, 17, 127, 128, 129, 240, 241, 255, 256} (256-key kernels, 241..256 the T1 forms) and
{257, 383, 384, 385, 496, 497, 511, 512} (512-key kernels); B = 2, two heads of 64; bf16 and fp16 operands.

test_per_element_bound, per T' and operand type, for p = 0, p = 0.1 hashed, and at T' <= 256 p = 0.1 with stored keep
bits and with bits drawn ahead:
  - |kernel - ref64| <= bound at every element of O (and the fp16 forward's bf16 copy), lse2 (log2 domain), delta,
    the fp32 gradient image dqkv and its bf16 image dqkv16; the worst |err| / bound per output is printed;
  - the keep mask of the reference is the numpy restatement of the hash; the stored and the drawn-ahead keep words
    decode to exactly that mask;
  - the paired-tile and the per-tile dK/dV kernels write bitwise-equal dqkv, dqkv16 (the paired form is bounded);
  - every output is a view between NaN-filled guard rows: the guards are still NaN after the launches and every
    element in range is finite (written, nothing left of the fill).
test_seed_epoch: the same under a device step counter (b2p_set_seed_epoch) at one T' per shape class, the reference
mask drawn under the restatement of b2p_seed_eff.
test_fp16_operands_that_are_no_bf16_numbers: the inputs above are bf16 numbers even in the fp16 mode, so the backward's
fp16 -> bf16 conversion of V, Q and K (to_b16) is exact on them; here qkv is rounded to fp16 directly, at one T' per
shape class, and the bound's residual terms of those operands carry weight.
test_batch_independence: with the batch-1 rows of qkv and dO set to NaN every batch-0 row of every output equals the
clean two-batch run bit for bit (a partial tile that read the next batch's rows and masked them by multiplication
would leak the NaN), in every dropout form and both operand types.

Measured on an MI355X, worst |err| / bound over the lengths, dropout forms and epoch cases of each kernel class (the
bound held at the first run: no term was added after it, and no multiplier exists to fit):
  class      operands  O      Ob     lse2   delta  dqkv   dqkv16
  T' <= 240  bf16      0.790  -      0.021  0.005  0.916  0.763
  T' <= 240  fp16      0.680  0.824  0.021  0.005  0.916  0.843
  241..256   bf16      0.797  -      0.021  0.006  0.752  0.721
  241..256   fp16      0.681  0.702  0.021  0.006  0.752  0.721
  257..512   bf16      0.798  -      0.022  0.006  0.718  0.660
  257..512   fp16      0.678  0.759  0.022  0.006  0.718  0.660
  fp16 operands that are no bf16 numbers (T' = 17 / 249 / 313): O 0.675, Ob 0.824, lse2 0.019, delta 0.183, dqkv 0.753,
  dqkv16 0.695 at the most.
The host emulation, which rounds at the 16-bit points only, reaches 0.916 on dqkv and 0.824 on Ob as well: the kernels'
16-bit roundings are where the derivation places them. lse2 and delta stay far below 1 because their bounds are
worst-case sums of fp32 roundings (64 products per score charged a whole ulp each) while the errors add like a random
walk; in the host test a key dropped in the last tile still exceeds the lse2 bound 90 times and more, scores off by
5 % 360 times and more, and an inverted keep bit the delta bound 110 times and more.
"""
import ctypes

import pytest
import torch

from tests import attn16_cases as C

pytestmark = pytest.mark.gpu

MODES = [pytest.param(False, id="bf16"), pytest.param(True, id="fp16")]


@pytest.mark.parametrize("half", MODES)
@pytest.mark.parametrize("T", C.T_ALL)
def test_per_element_bound(T, half):
    worst, fails = C.bound_case(T, half)
    assert not fails, (T, half, fails, worst)


@pytest.mark.parametrize("half", MODES)
@pytest.mark.parametrize("T", C.T_EPOCH)
def test_seed_epoch(T, half):
    Fn = C.fn()
    lib = Fn._lib.load()
    ctr = torch.full((1,), C.EPOCH, dtype=torch.int64, device="cuda")
    Fn._lib.check(lib.b2p_set_seed_epoch(ctypes.c_void_p(ctr.data_ptr())), "set_seed_epoch")
    try:
        worst, fails = C.bound_case(T, half, epoch=C.EPOCH, form_list=[f for f in C.forms(T) if f[1] > 0])
    finally:
        Fn._lib.check(lib.b2p_set_seed_epoch(None), "set_seed_epoch")
    assert not fails, (T, half, fails, worst)


@pytest.mark.parametrize("T", C.T_EPOCH)
def test_fp16_operands_that_are_no_bf16_numbers(T):
    worst, fails = C.bound_case(T, True, via_bf16=False)
    assert not fails, (T, fails, worst)


@pytest.mark.parametrize("T", C.T_ALL)
def test_batch_independence(T):
    for half in (False, True):
        qkv, dO = (x.cuda() for x in C.operands(T, half))
        qkv_n, dO_n = qkv.clone(), dO.clone()
        qkv_n[T:] = float("nan")
        dO_n[T:] = float("nan")
        for form, p in C.forms(T):
            clean = C.run(T, half, form, p, qkv, dO)
            clean.check()
            dirty = C.run(T, half, form, p, qkv_n, dO_n)
            dirty.check(nb=1)
            for name, (view, _, _) in clean.g.items():
                n0 = view.shape[0] // C.B       # batch 0: the first B-th of the leading dimension
                assert torch.equal(C.bits(view[:n0]), C.bits(dirty[name][:n0])), (T, half, form, name)
