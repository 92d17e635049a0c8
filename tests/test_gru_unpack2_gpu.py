"""b2p_gru_lane_unpack2 (csrc/gru16.hip): one pass over the backward's lane-native dgL writes both dgi (records
0, 1, 2) and dgh (records 0, 1, 3); it must equal the two b2p_gru_lane_permute calls it replaces, word for word,
and leave the rest of both destinations (here: NaN guards around them) alone."""
import numpy as np
import pytest
import torch

from tests.gru16_cases import Guarded

pytestmark = pytest.mark.gpu

MAP_GI, MAP_GH = 0xF210, 0x2F10


@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", [1, 17, 33])
@pytest.mark.parametrize("H", [32, 256])
def test_unpack2_equals_two_permutes(H, B, T, ndir):
    from wav2vec2forbrain_amd import _lib
    lib = _lib.load()
    st = _lib.stream_ptr()
    n_ln = int(lib.b2p_gru16_lane_floats(B, T, H, ndir, 4))
    g = torch.Generator().manual_seed(H + 7 * B + 31 * T + ndir)
    src = torch.randn(n_ln, generator=g).cuda()
    n_std = B * T * ndir * 3 * H
    gd = Guarded()
    ref = [gd.new(n_std), gd.new(n_std)]
    got = [gd.new(n_std), gd.new(n_std)]
    for dst, rmap in zip(ref, (MAP_GI, MAP_GH)):
        _lib.call("b2p_gru_lane_permute", src.data_ptr(), dst.data_ptr(), B, T, H, ndir, 4, 3, rmap, 0, st)
    _lib.call("b2p_gru_lane_unpack2", src.data_ptr(), got[0].data_ptr(), got[1].data_ptr(), B, T, H, ndir, 4, 3,
              MAP_GI, MAP_GH, st)
    torch.cuda.synchronize()
    gd.check()   # guards untouched, every destination fully written
    for r, o in zip(ref, got):
        assert np.array_equal(r.cpu().numpy().view(np.uint32), o.cpu().numpy().view(np.uint32))


def test_unpack2_rejects_bad_maps():
    from wav2vec2forbrain_amd import _lib
    lib = _lib.load()
    x = torch.zeros(int(lib.b2p_gru16_lane_floats(1, 1, 32, 1, 4)), device="cuda")
    y = torch.zeros(2, 3 * 32, device="cuda")
    assert lib.b2p_gru_lane_unpack2(x.data_ptr(), y[0].data_ptr(), y[1].data_ptr(), 1, 1, 32, 1, 4, 3, 0xF210, 0x3F10,
                                    _lib.stream_ptr()) != 0
    assert lib.b2p_gru_lane_unpack2(x.data_ptr(), y[0].data_ptr(), None, 1, 1, 32, 1, 4, 3, 0xF210, 0x2F10,
                                    _lib.stream_ptr()) != 0
