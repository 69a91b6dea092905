"""bench.py's plain run and its --dump-outputs / --full options: a plain run times the steps and prints the
line without the measurements that take runs of their own; --dump-outputs DIR writes the last timed step's
outputs as DIR/<name>.npy (float32 / float64, a fixed seeded sample of any array above 2^20 elements)."""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, str(ROOT))
import bench  # noqa: E402

DUMPED = {"params", "step_stats", "grad_norms", "train_stats", "actions", "logprobs", "values", "advantages",
          "returns"}


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_array_keeps_small_outputs_whole():
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()  # not contiguous
    out = bench.dump_array(x)
    assert out.dtype == np.float32 and np.array_equal(out, x.reshape(-1).numpy())
    d = bench.dump_array(np.linspace(0.0, 1.0, 5))
    assert d.dtype == np.float64 and np.array_equal(d, np.linspace(0.0, 1.0, 5))
    i = bench.dump_array(torch.tensor([[3, 1], [0, 2]], dtype=torch.int64))
    assert i.dtype == np.float32 and i.tolist() == [3.0, 1.0, 0.0, 2.0]


def test_dump_array_samples_large_outputs_at_fixed_positions():
    n = bench.DUMP_MAX_ELEMS + 4097
    x = torch.arange(n, dtype=torch.float32)  # exact in fp32: n < 2^24, so each value is its own position
    a, b = bench.dump_array(x), bench.dump_array(x.clone())
    assert a.shape == (bench.DUMP_MAX_ELEMS,) and a.dtype == np.float32
    assert np.array_equal(a, b)  # the same positions every time
    assert np.all(np.diff(a) >= 0) and a[0] >= 0 and a[-1] < n
    assert a[-1] - a[0] > 0.99 * n  # spread over the whole array, not a prefix
    assert 9 * a.nbytes <= 64 << 20  # every dumped array at the cap still fits the 64 MB budget
    assert len(DUMPED) == 9


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_step(tmp_path):
    """One plain run at 64 envs (128 x 64 rows, 32 minibatches x 20 epochs per step): the line carries the
    headline keys with ms_per_step consistent with value, none of the --full measurements, and the dump
    holds the nine arrays at their full sizes."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--num-envs", "64", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["metric"].startswith("env-steps/sec") and line["steps"] == 2 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    np.testing.assert_allclose(line["ms_per_step"], 128 * 64 / line["value"] * 1e3, rtol=1e-3)
    assert line["full"] is False
    assert line["cpu_baseline"] is None and line["roofline_gae"] is None
    assert line["roofline_gae_bandwidth_regime"] is None
    assert line["roofline"]["launches_timed"] == 2 * 20  # read off the timed steps themselves

    assert {p.stem for p in out.iterdir()} == DUMPED and all(p.suffix == ".npy" for p in out.iterdir())
    arrs = {n: np.load(out / (n + ".npy"), allow_pickle=False) for n in DUMPED}
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    for n, a in arrs.items():
        assert a.dtype in (np.float32, np.float64) and a.ndim == 1 and np.all(np.isfinite(a)), n
    for n in ("actions", "logprobs", "values", "advantages", "returns"):
        assert arrs[n].size == 128 * 64, n
    # the CartPole actor-critic: [4 -> 64 -> 64 -> 2] actor and [4 -> 64 -> 64 -> 1] critic
    assert arrs["params"].size == (4 * 64 + 64) * 2 + (64 * 64 + 64) * 2 + (64 * 2 + 2) + (64 + 1)
    assert arrs["grad_norms"].size == 20 * 32 and arrs["step_stats"].size % (20 * 32) == 0
    assert set(np.unique(arrs["actions"])) <= {0.0, 1.0}
    # returns = advantages + values (GAE), all three from the last step's rollout
    np.testing.assert_allclose(arrs["returns"], arrs["advantages"] + arrs["values"], rtol=1e-5, atol=1e-5)
