"""bench.py --dump-outputs (CPU): the files it writes are float32 .npy, stay inside the byte budget,
and an array larger than its share is written as the same sample in every run."""
import os

import numpy as np
import torch

import bench


def test_write_outputs_float32_within_budget_and_repeatable(tmp_path):
    g = torch.Generator().manual_seed(3)
    arrays = {"loss": torch.randn(1, generator=g, dtype=torch.float64),
              "logits": torch.randn(4, 7, 5, generator=g).to(torch.bfloat16),
              "big": torch.randn(5000, generator=g)}
    budget = 3 * 4 * 1000     # 1000 float32 elements for each of the three arrays
    a, b = tmp_path / "a", tmp_path / "b"
    bench.write_outputs(str(a), arrays, budget=budget)
    bench.write_outputs(str(b), arrays, budget=budget)
    assert sorted(os.listdir(a)) == ["big.npy", "logits.npy", "loss.npy"]
    got = {n: np.load(a / f"{n}.npy") for n in arrays}
    assert all(v.dtype == np.float32 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= budget
    # arrays within their share are written whole, in their own shape
    assert got["loss"].shape == (1,) and got["loss"][0] == np.float32(arrays["loss"][0])
    assert np.array_equal(got["logits"], arrays["logits"].float().numpy())
    # the larger one: a sample of its own elements, identical from run to run
    assert got["big"].shape == (1000,)
    assert np.isin(got["big"], arrays["big"].numpy()).all()
    assert len(np.unique(got["big"])) > 800
    for n in arrays:
        assert np.array_equal(got[n], np.load(b / f"{n}.npy"))


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    """A plain command line turns every leg but the timed steps off; --full leaves them on."""
    seen = {}

    def fake_timed_run(kind, args, *a, **kw):
        seen["args"], seen["dump"] = args, kw.get("dump")
        raise SystemExit(0)

    monkeypatch.setattr(bench, "timed_run", fake_timed_run)
    from wav2vec2forbrain_amd import build_lib
    monkeypatch.setattr(build_lib, "ensure_built", lambda: None)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    legs = ("no_cpu_baseline", "no_parity", "no_roofline", "no_conformer", "no_extra")

    def read_only_tree():   # the library is there (conftest built it), the tree cannot be written to
        raise PermissionError(13, "Permission denied", "build/obj/.lock")

    for argv, off in ((["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", "d"], True),
                      (["--full", "--steps", "3"], False)):
        if not off:     # the second run: bench goes on with the library that is there
            monkeypatch.setattr(build_lib, "ensure_built", read_only_tree)
        seen.clear()
        monkeypatch.setattr("sys.argv", ["bench.py", *argv])
        try:
            bench.main()
        except SystemExit:
            pass
        assert seen["args"].steps == 3
        assert [getattr(seen["args"], k) for k in legs] == [off] * 5
        assert seen["dump"] == ("d" if off else None)
