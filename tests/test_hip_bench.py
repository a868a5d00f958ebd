"""A plain `bench.py` run on the GPU (-m gpu): exactly --steps timed steps in one block, the headline fields and nothing
that only --full measures, and --dump-outputs files that are the same from run to run (seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _plain(dump):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--batch", "4", "--points", "256", "--dump-outputs", dump],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_times_exactly_its_steps_and_dumps_its_outputs(tmp_path):
    j = _plain(str(tmp_path / "a"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j, k
    assert j["unit"] == "pairs/s" and j["higher_is_better"] is True and j["dtype"] == "f32" and j["steps"] == 4
    tb = j["timed_blocks"]
    assert tb["count"] == 1 and tb["steps_per_block"] == 4 and len(tb["seconds"]) == 1
    assert abs(j["ms_per_step"] * 4 * 1e-3 - tb["seconds"][0]) <= 1e-6          # (the block's seconds are rounded to 1 us)
    assert j["value"] == pytest.approx(4 * 4 / (j["ms_per_step"] * 4 * 1e-3), rel=1e-9)
    for k in ("roofline", "stages", "accounted_frac", "other_configs", "cpu_baseline", "parity_ledger"):
        assert k not in j, k
    _plain(str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in bench.DUMP_NAMES)
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        np.testing.assert_array_equal(a, b, err_msg=n)
    assert np.load(tmp_path / "a" / "rotation_ab.npy").shape == (4, 3, 3)
    assert np.load(tmp_path / "a" / "translation_ab.npy").shape == (4, 3)


@pytest.mark.parametrize("extra", [[], ["--full", "--min-seconds", "0.05"]], ids=["plain", "full"])
def test_measure_runs_exactly_steps_per_timed_block(monkeypatch, extra):
    """Every vcrnetIter call of bench.measure counted: one initialisation call, --warmup warm-up steps, then --steps steps
    per timed block -- a plain run has exactly one block, --full repeats it for --min-seconds."""
    from types import SimpleNamespace
    import torch
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import module
    calls = []
    real = module.vcrnetIter

    def counted(*args, **kw):
        calls.append(1)
        return real(*args, **kw)

    monkeypatch.setattr(module, "vcrnetIter", counted)
    a = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2", "--batch", "2", "--points", "256"] + extra)
    ctx = SimpleNamespace(world=1, rank=0, dev=torch.device("cuda", 0), dist=None, ndev=torch.cuda.device_count(), rccl_log=None)
    line = bench.measure(a, ctx, a.min_seconds)
    blocks = line["timed_blocks"]["count"]
    assert len(calls) == 1 + 2 + 5 * blocks
    if extra:
        assert blocks >= 1 and "roofline" in line
    else:
        assert blocks == 1 and "roofline" not in line
    assert line["steps"] == 5 and len(line["timed_blocks"]["seconds"]) == blocks
