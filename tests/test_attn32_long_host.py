"""The long-class kernels of csrc/attn32.hip (257 <= T' <= 512) as the compiler built them for gfx950: every
instantiation is present and none uses scratch (a score tile or an accumulator spilled to memory would be
re-read in the innermost loop)."""
import pytest


@pytest.mark.timeout(600)
def test_no_scratch_in_any_long_kernel():
    from wav2vec2forbrain_amd import build_lib
    scratch = {k: v for k, v in build_lib.audit_scratch("attn32.hip").items() if "attn32_long_" in k}
    for kern in ("attn32_long_fwd_k", "attn32_long_bwd_dq_k", "attn32_long_bwd_dkv_k"):
        for drop in (0, 1):
            hit = [k for k in scratch if f"{kern}ILb{drop}E" in k]
            assert len(hit) == 1, (kern, drop, sorted(scratch))
            assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
