"""bench.py's own options, without a GPU: --full is off by default, --steps is the number of timed steps and at least
one, and --dump-outputs keeps within its byte budget by writing a fixed sample of clips."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_a_plain_run_is_not_a_full_one_and_steps_must_be_positive():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_writes_float32_and_samples_above_the_budget(tmp_path, monkeypatch):
    rows = torch.arange(40 * 6, dtype=torch.float32).reshape(40, 6)
    bench.dump_outputs(str(tmp_path / "small"), "features", rows)
    assert sorted(os.listdir(tmp_path / "small")) == ["features.npy"]
    got = np.load(tmp_path / "small" / "features.npy")
    assert got.dtype == np.float32 and np.array_equal(got, rows.numpy())

    raster = (torch.arange(50 * 3 * 4) % 2).to(torch.uint8).reshape(50, 3, 4)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1024 + 20 * (3 * 4 * 4 + 8))     # room for 20 of the 50 clips
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "rasters", raster)
    idx = np.load(tmp_path / "a" / "rasters_index.npy")
    got = np.load(tmp_path / "a" / "rasters.npy")
    assert idx.dtype == np.float64 and len(idx) == 20 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < 50
    assert got.dtype == np.float32 and np.array_equal(got, raster.numpy()[idx.astype(np.int64)].astype(np.float32))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_LIMIT_BYTES
    for name in ("rasters.npy", "rasters_index.npy"):                # the sample is fixed: the same clips every run
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name))
