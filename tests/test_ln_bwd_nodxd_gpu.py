"""The dropout-input form of the LayerNorm backward without its fp32 image (b2p_layernorm_bwd_flags with
B2P_LNB_IN_DROP and dx_dropped = NULL; functional._ln_bwd16(want_dxd=False)) against the form that
writes the image: dx, d16 and dgamma / dbeta / dbias_in are bit for bit the same, returned directly and
left as lazy block partials, for every accumulator form, both LayerDrop gates open and closed and
in-dropout p = 0 and 0.1; no rows x cols fp32 tensor is allocated for the image.

The reference is the existing form itself (tests/test_layernorm_ops_gpu.py ties it to float64)."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = ((37, 256), (64, 768), (33, 1024))
SEED1, SEED2 = 0x5EED0001, 0x5EED0002


def _inputs(rows, cols):
    g = torch.Generator().manual_seed(7919 * rows + 31 * cols)
    mk = lambda *s: torch.randn(*s, generator=g).cuda()
    x = mk(rows, cols) * 1.5 + 0.3
    return dict(x=x, gamma=mk(cols), dy=mk(rows, cols), acc1=mk(rows, cols), acc2=mk(rows, cols),
                mean=x.mean(1), rstd=(x.var(1, unbiased=False) + 1e-5).rsqrt())


def _gate(v):
    return None if v is None else torch.tensor([v], dtype=torch.int32, device="cuda")


def _run(Fn, t, want_dxd, a1, a2, gates, p_in, lazy):
    """One _ln_bwd16 call; gates = (dy_gate, acc2_gate) values (None: no gate). lazy: the three parameter
    gradients are left as block partials (their owners registered as deferred frozen parameters)."""
    cols = t["x"].shape[1]
    dbias = torch.empty(cols, device="cuda")
    kw = dict(need_params=True, dx_accum=t["acc1"] if a1 else None, drop_p=0.1, seed=SEED1, in_drop_p=p_in,
              in_seed=SEED2, dbias_in=dbias, dx_accum2=t["acc2"] if a2 else None, dy_gate=_gate(gates[0]),
              acc2_gate=_gate(gates[1]) if a2 else None, want_dxd=want_dxd)
    if lazy:
        owners = tuple(torch.nn.Parameter(torch.zeros(cols, device="cuda")) for _ in range(3))
        Fn._Deferred.ids.update(id(p) for p in owners)
        try:
            dx, dg, db, dxd, d16, dbi = Fn._ln_bwd16(t["dy"], t["x"], t["gamma"], t["mean"], t["rstd"], lazy=owners, **kw)
        finally:
            for p in owners:
                Fn._Deferred.ids.discard(id(p))
        assert all(isinstance(g, Fn.ColsumParts) for g in (dg, db, dbi))
        parts = [g.parts.clone() for g in (dg, db, dbi)]
        dg, db, dbi = (g.materialize() for g in (dg, db, dbi))
    else:
        dx, dg, db, dxd, d16 = Fn._ln_bwd16(t["dy"], t["x"], t["gamma"], t["mean"], t["rstd"], **kw)
        dbi, parts = dbias, []
    torch.cuda.synchronize()
    return dict(dx=dx, d16=d16, dg=dg, db=db, dbi=dbi, dxd=dxd, parts=parts)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_no_image_form_keeps_every_other_output(rows, cols):
    from wav2vec2forbrain_amd import functional as Fn
    t = _inputs(rows, cols)
    cases = 0
    # gates: none, both open (1), both closed (0)
    for a1, a2, gv, p_in, lazy in itertools.product((False, True), (False, True), (None, 1, 0), (0.0, 0.1),
                                                    (False, True)):
        old = _run(Fn, t, True, a1, a2, (gv, gv), p_in, lazy)
        new = _run(Fn, t, False, a1, a2, (gv, gv), p_in, lazy)
        tag = (rows, cols, a1, a2, gv, p_in, lazy)
        assert old["dxd"] is not None and old["dxd"].shape == (rows, cols), tag
        assert new["dxd"] is None, tag
        for k in ("dx", "d16", "dg", "db", "dbi"):
            assert _same(old[k], new[k]), (k, tag)
        for po, pn in zip(old["parts"], new["parts"]):
            assert _same(po, pn), tag
        # the form is really the dropout-input one: d16 is the bf16 image of the dropped dx
        assert _same(new["d16"], old["dxd"].to(torch.bfloat16)), tag
        cases += 1
    assert cases == 48


def test_no_image_sized_allocation():
    """The call without the image allocates one rows x cols fp32 tensor less than the call with it."""
    from wav2vec2forbrain_amd import functional as Fn
    rows, cols = 64, 768
    t = _inputs(rows, cols)
    peaks = {}
    for want in (True, False):
        _run(Fn, t, want, True, False, (None, None), 0.1, False)   # warm the allocator's small pools
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = _run(Fn, t, want, True, False, (None, None), 0.1, False)
        peaks[want] = torch.cuda.max_memory_allocated() - base
        del out
    image = rows * cols * 4
    assert peaks[True] - peaks[False] >= image, peaks
    assert peaks[False] < 2 * image + rows * cols * 2 + (1 << 20), peaks   # dx, d16, workspace: no second image


def test_c_entry_point_flag_contract():
    """flags = 0 is b2p_layernorm_bwd_gated: with dx_dropped = NULL the dropout-input form stays off
    (d16 = bf16(dx)); an unknown flag is refused."""
    from wav2vec2forbrain_amd import _lib
    from wav2vec2forbrain_amd import functional as Fn
    rows, cols = 37, 256
    t = _inputs(rows, cols)
    ws = torch.empty(int(_lib.load().b2p_layernorm_bwd_workspace(rows, cols)), device="cuda")
    dx = torch.empty(rows, cols, device="cuda")
    d16 = torch.empty(rows, cols, device="cuda", dtype=torch.bfloat16)
    p = Fn._p

    def call(flags):
        return _lib.load().b2p_layernorm_bwd_flags(p(t["dy"]), p(t["x"]), p(t["gamma"]), p(t["mean"]), p(t["rstd"]), p(dx),
                                                   None, None, rows, cols, None, None, 0.0, 0, None, 0.1, SEED2, None,
                                                   p(d16), None, None, flags, p(ws), Fn._st())

    assert call(0) == 0
    torch.cuda.synchronize()
    assert _same(d16, dx.to(torch.bfloat16))
    assert call(1) == 0
    torch.cuda.synchronize()
    assert not _same(d16, dx.to(torch.bfloat16))
    assert call(2) != 0
