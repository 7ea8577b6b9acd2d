"""bench.py's command line: a plain run prints the headline line only, --full adds the other measurements and checks,
--dump-outputs writes the last timed step's outputs as .npy files (float32, at most 64 MB in all, the same elements in
every run with the same arguments)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*argv, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), env=env, capture_output=True,
                          text=True, timeout=timeout)


def _line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_float32_within_limit_and_repeatable(tmp_path):
    g = torch.Generator().manual_seed(0)
    outs = {"big": torch.randn(3000, 500, generator=g), "half": torch.randn(40, 7, generator=g).half(),
            "wide": torch.randn(10, dtype=torch.float64, generator=g)}
    limit = 2_000_000
    info = bench.dump_outputs(str(tmp_path / "a"), outs, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), outs, limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "half.npy", "wide.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= limit
    big = np.load(tmp_path / "a" / "big.npy")
    assert big.dtype == np.float32 and 0 < big.size < outs["big"].numel()
    assert info["big"]["shape"] == [3000, 500] and info["big"]["written"].startswith("sample")
    # the sample is the seeded index set of the docstring (seed = position 0), the same in every run
    idx = np.unique(np.random.default_rng(0).integers(0, outs["big"].numel(), (limit - 4096 * 3) // 3 // 4))
    assert np.array_equal(big, outs["big"].reshape(-1).numpy()[idx])
    half = np.load(tmp_path / "a" / "half.npy")
    assert half.dtype == np.float32 and half.shape == (40, 7) and info["half"]["written"] == "all"
    assert np.array_equal(half, outs["half"].float().numpy())
    wide = np.load(tmp_path / "a" / "wide.npy")
    assert wide.dtype == np.float64 and np.array_equal(wide, outs["wide"].numpy())
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_bench_options_and_step_count_checked():
    h = _run_bench("--help", timeout=240)
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    r = _run_bench("--steps", "0", timeout=240)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_outputs(dev, tmp_path):
    """A plain run: the headline fields, the requested number of timed steps, none of the --full blocks, and the four
    outputs of the last timed step, finite, the same in a second run with the same arguments."""
    common = ("--steps", "3", "--warmup", "1", "--batch", "2", "--points", "4096")
    line = _line(_run_bench(*common, "--dump-outputs", str(tmp_path / "a")))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["unit"] == "frames/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["value"] > 0 and abs(line["value"] - 2 * 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    for k in ("roofline", "ops", "extras", "cpu_baseline"):
        assert k not in line, k
    assert "verified" not in line["config"]
    assert sorted(line["outputs_dumped"]) == sorted(bench.Bench.OUTPUTS)
    _line(_run_bench(*common, "--dump-outputs", str(tmp_path / "b")))
    for name in bench.Bench.OUTPUTS:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), name
        info = line["outputs_dumped"][name]
        if info["written"] == "all":
            assert list(a.shape) == info["shape"], name
        else:
            assert a.ndim == 1 and 0 < a.size < np.prod(info["shape"]), name
        assert np.array_equal(a, b), f"{name}: differs between two runs with the same arguments"


@pytest.mark.gpu
def test_full_run_keeps_the_other_measurements(dev):
    line = _line(_run_bench("--full", "--steps", "3", "--warmup", "1", "--batch", "2", "--points", "4096",
                            "--no-cpu-baseline", "--no-extras"))
    assert line["steps"] == 3 and line["config"]["verified"]["vs_serial"] == "bit-equal"
    for k in ("roofline", "roofline_hbm", "ops", "ball_query_plus_group", "pdm_neck_forms", "extras"):
        assert k in line, k
