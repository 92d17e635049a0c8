"""C ABI of the persistent exact-fp32 GRU recurrence (csrc/gru32.hip) without a device: the symbols are
exported and bound, b2p_gru32_supported / b2p_gru32_workspace state the shape class and the workspace, and
every argument error is reported before any HIP call (the pointers below are never dereferenced)."""
import ctypes

import pytest

FAKE = 0x10000   # a non-NULL, 16-byte aligned address: validation fails before it is used


def _lib():
    from wav2vec2forbrain_amd import _lib
    return _lib, _lib.load()


def test_symbols_exported_and_bound():
    _l, lib = _lib()
    arity = {"b2p_gru32_supported": 1, "b2p_gru32_workspace": 3, "b2p_gru_fwd32": 12, "b2p_gru_bwd32": 14}
    for name, n in arity.items():
        assert name in _l.exported_symbols()
        fn = getattr(lib, name)     # AttributeError when the library does not export it
        assert len(fn.argtypes) == n
        assert fn.restype is (ctypes.c_int64 if name == "b2p_gru32_workspace" else ctypes.c_int32)


@pytest.mark.parametrize("H,ok", [(256, 1), (512, 1), (0, 0), (100, 0), (8192, 0)])
def test_supported(H, ok):
    _l, lib = _lib()
    assert lib.b2p_gru32_supported(H) == ok


@pytest.mark.parametrize("H", [256, 512])
@pytest.mark.parametrize("ndir", [1, 2])
def test_workspace(H, ndir):
    _l, lib = _lib()
    prev = 0
    for B in (1, 8, 16, 17, 32, 33, 64, 65, 200):
        n = lib.b2p_gru32_workspace(B, H, ndir)
        assert n > 0 and n % 16 == 0 and n >= prev, (B, n, prev)
        prev = n
    assert lib.b2p_gru32_workspace(17, H, ndir) > lib.b2p_gru32_workspace(16, H, ndir)   # one more batch group


def _fwd(lib, p=FAKE, ws=FAKE, H=512, ndir=2, B=4, T=3):
    return lib.b2p_gru_fwd32(p, FAKE, None, None, FAKE, FAKE, ws, B, T, H, ndir, None)


def _bwd(lib, p=FAKE, ws=FAKE, H=512, ndir=2, B=4, T=3):
    return lib.b2p_gru_bwd32(p, FAKE, FAKE, FAKE, None, FAKE, FAKE, None, ws, B, T, H, ndir, None)


@pytest.mark.parametrize("call", [_fwd, _bwd])
@pytest.mark.parametrize("kw,word", [(dict(p=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(H=100), b"hidden size 100"),
                                     (dict(H=8192), b"hidden size 8192"), (dict(ndir=3), b"ndir"), (dict(ndir=0), b"ndir"),
                                     (dict(ws=FAKE + 8), b"16-byte aligned")])
def test_argument_validation_without_device(call, kw, word):
    _l, lib = _lib()
    assert call(lib, **kw) != 0
    err = lib.b2p_last_error()
    assert b"gru32" in err and word in err, err


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_empty_batch_or_time(call):
    _l, lib = _lib()
    assert call(lib, B=0) == 0     # nothing to do: no launch, no error
    assert call(lib, T=0) == 0
