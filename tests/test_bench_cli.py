"""bench.py's command line without a GPU: what a plain run does and what only --full adds, and --dump-outputs' files."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_times_one_block_and_full_keeps_the_old_protocol():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.min_seconds == 0.0 and a.steps == 7 and a.dump_outputs is None
    f = bench.parse(["--full"])
    assert f.full and f.min_seconds == 12.0
    assert bench.parse(["--min-seconds", "3"]).min_seconds == 3.0
    assert bench.parse(["--full", "--stages"]).stages
    with pytest.raises(SystemExit):
        bench.parse(["--stages"])                    # the per-launch table needs the events only --full records
    # the extra knobs do not make a run a non-headline one
    assert bench.is_headline(bench.parse(["--full", "--dump-outputs", "x"]))


def test_dump_outputs_writes_float_arrays(tmp_path):
    g = torch.Generator().manual_seed(0)
    out = (torch.randn(2, 3, 10, generator=g), torch.randn(2, 3, 10, generator=g), torch.randn(2, 3, 3, generator=g),
           torch.randn(2, 3, generator=g), torch.randn(2, 3, 3, generator=g, dtype=torch.float64), torch.arange(6).view(2, 3))
    pose = torch.randn(4, 12, generator=g)
    bench.dump_outputs(str(tmp_path), out, pose)
    names = sorted(f[:-4] for f in os.listdir(tmp_path))
    assert names == sorted(bench.DUMP_NAMES + ("poses_all_ranks",))
    for n, t in list(zip(bench.DUMP_NAMES, out)) + [("poses_all_ranks", pose)]:
        v = np.load(os.path.join(tmp_path, n + ".npy"))
        assert v.dtype in (np.float32, np.float64) and v.shape == tuple(t.shape)
        np.testing.assert_array_equal(v, t.numpy().astype(v.dtype))
    assert np.load(os.path.join(tmp_path, "rotation_ba.npy")).dtype == np.float64
    assert np.load(os.path.join(tmp_path, "translation_ba.npy")).dtype == np.float64      # integers as float64


def test_dump_outputs_samples_what_exceeds_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    big = torch.randn(16, 3, 1024, generator=torch.Generator().manual_seed(1))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), (big, torch.ones(2, 3)))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["corr_k.npy", "src_k.index.npy", "src_k.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 4096
    idx = np.load(tmp_path / "a" / "src_k.index.npy").astype(np.int64)
    v = np.load(tmp_path / "a" / "src_k.npy")
    np.testing.assert_array_equal(v, big.numpy().reshape(-1)[idx])
    for f in files:                                  # the sample is fixed: the same elements every run
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
