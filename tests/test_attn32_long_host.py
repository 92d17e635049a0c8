"""The kernels of csrc/attn32.hip (both shape classes, T' <= 512) as the compiler built them for gfx950: every
instantiation is present exactly once and none uses scratch (a score tile or an accumulator spilled to memory
would be re-read in the innermost loop)."""
import pytest

# mangled template arguments: ILi<chunks>ELb<drop>EE for the kernels templated on the class, ILb<drop>EE for the
# two dQ bodies
INSTANCES = ([f"attn32_fwd_kILi{nc}ELb{d}EE" for nc in (1, 2) for d in (0, 1)]
             + [f"attn32_bwd_dkv_kILi{nc}ELb{d}EE" for nc in (1, 2) for d in (0, 1)]
             + [f"{k}ILb{d}EE" for k in ("15attn32_bwd_dq_k", "20attn32_long_bwd_dq_k") for d in (0, 1)])


@pytest.mark.timeout(600)
def test_no_scratch_in_any_kernel():
    from wav2vec2forbrain_amd import build_lib
    scratch = build_lib.audit_scratch("attn32.hip")
    assert len(scratch) == len(INSTANCES) == 12, sorted(scratch)     # nothing else in the file is a kernel
    for inst in INSTANCES:
        hit = [k for k in scratch if inst in k]
        assert len(hit) == 1, (inst, sorted(scratch))
        assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
