"""C ABI of the persistent exact-fp32 GRU recurrence (csrc/gru32.hip) at hidden size 1024, without a device:
the shape class, the workspace against the formula of include/b2p_hip.h, the 256 / 512 workspaces against the
values of the build before H = 1024 existed, and the argument errors (the pointers are never dereferenced)."""
import pytest

FAKE = 0x10000   # a non-NULL, 16-byte aligned address: validation fails before it is used
BATCHES = (1, 8, 16, 17, 32, 33, 64, 65)
# b2p_gru32_workspace(B, H, ndir) for B in BATCHES, recorded from the build that had 256 and 512 only
BEFORE = {(256, 1): (524432, 524432, 524432, 1048848, 1048848, 1573264, 2097680, 2622096),
          (256, 2): (1048848, 1048848, 1048848, 2097680, 2097680, 3146512, 4195344, 5244176),
          (512, 1): (2097296, 2097296, 2097296, 4194576, 4194576, 6291856, 8389136, 10486416),
          (512, 2): (4194576, 4194576, 4194576, 8389136, 8389136, 12583696, 16778256, 20972816)}


def _lib():
    from wav2vec2forbrain_amd import _lib
    return _lib.load()


def _formula(B, H, nd):
    """include/b2p_hip.h: 16 B of fail words, S member ids of 8 B per recurrence (S = 16, at H = 1024 32), then per
    recurrence 2 slots of P x P x 512 granules of 8 B (P = H / 32), for ndir * ceil(B / 16) recurrences."""
    g, P, S = nd * ((B + 15) // 16), H // 32, 32 if H == 1024 else 16
    return 16 + g * S * 8 + g * 2 * P * P * 512 * 8


def test_supported():
    lib = _lib()
    assert lib.b2p_gru32_supported(1024) == 1
    assert lib.b2p_gru32_supported(768) == 0 and lib.b2p_gru32_supported(2048) == 0


@pytest.mark.parametrize("nd", [1, 2])
def test_workspace_1024(nd):
    lib = _lib()
    sizes = [int(lib.b2p_gru32_workspace(B, 1024, nd)) for B in BATCHES]
    for B, n, prev in zip(BATCHES, sizes, [0] + sizes):
        assert n > 0 and n % 16 == 0 and n >= prev, (B, n, prev)
        assert n == _formula(B, 1024, nd), (B, n)
    assert sizes[BATCHES.index(17)] > sizes[BATCHES.index(16)]   # one more batch group
    assert int(lib.b2p_gru32_workspace(8, 1024, 3)) == 0 and int(lib.b2p_gru32_workspace(8, 768, 2)) == 0


@pytest.mark.parametrize("H,nd", sorted(BEFORE))
def test_workspace_256_512_unchanged(H, nd):
    lib = _lib()
    got = tuple(int(lib.b2p_gru32_workspace(B, H, nd)) for B in BATCHES)
    assert got == BEFORE[(H, nd)]
    assert got == tuple(_formula(B, H, nd) for B in BATCHES)


def _fwd(lib, H=1024, B=4, T=3):
    return lib.b2p_gru_fwd32(FAKE, FAKE, None, None, FAKE, FAKE, FAKE, B, T, H, 2, None)


def _bwd(lib, H=1024, B=4, T=3):
    return lib.b2p_gru_bwd32(FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, None, FAKE, B, T, H, 2, None)


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_unsupported_size_names_it_and_lists_1024(call):
    lib = _lib()
    assert call(lib, H=768) != 0
    err = lib.b2p_last_error()
    assert b"gru32" in err and b"hidden size 768" in err and b"256, 512 or 1024" in err, err


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_empty_batch_or_time(call):
    lib = _lib()
    assert call(lib, B=0) == 0     # nothing to do: no launch, no error
    assert call(lib, T=0) == 0
