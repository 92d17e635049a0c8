"""C ABI of the fused exact-fp32 attention (csrc/attn32.hip) without a device: the symbols are exported and
bound, b2p_attn32_supported states the shape class, and every argument error is reported before any HIP
call (the pointers below are never dereferenced)."""
import ctypes

import pytest

FAKE = 0x10000   # a non-NULL, 16-byte aligned address: validation fails before it is used


def _lib():
    from wav2vec2forbrain_amd import _lib
    return _lib, _lib.load()


def test_symbols_exported_and_bound():
    _l, lib = _lib()
    for name in ("b2p_attn32_supported", "b2p_attn32_fwd", "b2p_attn32_bwd"):
        assert name in _l.exported_symbols()
        fn = getattr(lib, name)     # AttributeError when the library does not export it
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == {"b2p_attn32_supported": 2, "b2p_attn32_fwd": 11,
                                                                     "b2p_attn32_bwd": 13}[name]


@pytest.mark.parametrize("T,dh,ok", [(256, 64, 1), (1, 64, 1), (249, 64, 1), (257, 64, 0), (0, 64, 0), (249, 32, 0)])
def test_supported(T, dh, ok):
    _l, lib = _lib()
    assert lib.b2p_attn32_supported(T, dh) == ok
    from wav2vec2forbrain_amd import functional as Fn
    assert Fn.attn32_ok(T, dh) == bool(ok)


def _fwd(lib, qkv, T, dh, B=2, nh=2):
    return lib.b2p_attn32_fwd(qkv, FAKE, FAKE, B, T, nh, dh, 0.125, 0.0, 1, None)


def _bwd(lib, qkv, T, dh, B=2, nh=2):
    return lib.b2p_attn32_bwd(qkv, FAKE, FAKE, FAKE, FAKE, B, T, nh, dh, 0.125, 0.0, 1, None)


@pytest.mark.parametrize("call", [_fwd, _bwd])
@pytest.mark.parametrize("qkv,T,dh,word", [(FAKE, 17, 32, b"head size 64"), (FAKE, 257, 64, b"T <= 256"),
                                           (None, 17, 64, b"NULL")])
def test_argument_validation_without_device(call, qkv, T, dh, word):
    _l, lib = _lib()
    assert call(lib, qkv, T, dh) != 0
    err = lib.b2p_last_error()
    assert b"attn32" in err and word in err, err


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_index_bound_and_empty_batch(call):
    _l, lib = _lib()
    # B * heads * T * TP must stay below 2^32: 2048 * 32 * 256 * 256 = 2^32
    assert call(lib, FAKE, 256, 64, B=2048, nh=32) != 0
    assert b"attn32" in lib.b2p_last_error() and b"2^32" in lib.b2p_last_error()
    assert call(lib, FAKE, 256, 64, B=0) == 0     # nothing to do: no launch, no error
