"""C ABI of the long class (257 <= T' <= 512) of the fused exact-fp32 attention (csrc/attn32.hip) without a
device: the symbols are exported and bound, b2p_attn32_long_supported states the shape class, and every
argument error is reported with its bound before any HIP call (the pointers below are never dereferenced)."""
import ctypes

import pytest

FAKE = 0x10000   # a non-NULL, 16-byte aligned address: validation fails before it is used
NARGS = {"b2p_attn32_long_supported": 2, "b2p_attn32_long_fwd": 11, "b2p_attn32_long_bwd": 13}


def _lib():
    from wav2vec2forbrain_amd import _lib
    return _lib, _lib.load()


def test_symbols_exported_and_bound():
    _l, lib = _lib()
    for name, n in NARGS.items():
        assert name in _l.exported_symbols()
        fn = getattr(lib, name)     # AttributeError when the library does not export it
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == n
    # the argument lists are the 256 class's
    assert lib.b2p_attn32_long_fwd.argtypes == lib.b2p_attn32_fwd.argtypes
    assert lib.b2p_attn32_long_bwd.argtypes == lib.b2p_attn32_bwd.argtypes


@pytest.mark.parametrize("T,dh,ok", [(256, 64, 0), (257, 64, 1), (512, 64, 1), (513, 64, 0), (313, 32, 0)])
def test_supported(T, dh, ok):
    _l, lib = _lib()
    assert lib.b2p_attn32_long_supported(T, dh) == ok
    from wav2vec2forbrain_amd import functional as Fn
    assert Fn.attn32_long_ok(T, dh) == bool(ok)


def _fwd(lib, qkv=FAKE, T=313, dh=64, B=2, nh=2, p=0.0):
    return lib.b2p_attn32_long_fwd(qkv, FAKE, FAKE, B, T, nh, dh, 0.125, p, 1, None)


def _bwd(lib, qkv=FAKE, T=313, dh=64, B=2, nh=2, p=0.0):
    return lib.b2p_attn32_long_bwd(qkv, FAKE, FAKE, FAKE, FAKE, B, T, nh, dh, 0.125, p, 1, None)


@pytest.mark.parametrize("call", [_fwd, _bwd])
@pytest.mark.parametrize("kw,word", [(dict(qkv=None), b"NULL"), (dict(dh=32), b"head size 64"),
                                     (dict(T=256), b"257 <= T <= 512"), (dict(T=513), b"257 <= T <= 512"),
                                     (dict(nh=0), b"heads > 0"), (dict(p=1.0), b"0 <= drop_p < 1"),
                                     (dict(p=-0.1), b"0 <= drop_p < 1"),
                                     # B * heads * T * TP must stay below 2^32: 512 * 32 * 512 * 512 = 2^32
                                     (dict(T=512, B=512, nh=32), b"2^32")])
def test_argument_validation_without_device(call, kw, word):
    _l, lib = _lib()
    assert call(lib, **kw) != 0
    err = lib.b2p_last_error()
    assert b"attn32_long" in err and word in err, err


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_empty_batch(call):
    _l, lib = _lib()
    assert call(lib, B=0) == 0     # nothing to do: no launch, no error
