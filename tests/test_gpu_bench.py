"""bench.py as the driver runs it on one GPU: a plain run carries only the headline figure and
writes --dump-outputs; --full adds the roofline block and the parity leg. The dumped frame is what
the timed path returned after its last step: one context accumulates warmup + steps, so it must
equal one render of those samples."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bdpt_amd as B
from _util import REPO

pytestmark = pytest.mark.gpu

W, H, SPP, M, STEPS, WARM = 160, 120, 4, 5, 2, 1


@pytest.fixture(scope="module")
def single_render():
    sc = B.load_dae(os.path.join(REPO, "scenes", "CBspheres.dae"), W, H)
    pt = B.BidirectionalPathTracer(sc, W, H, SPP, M, seed=5489)
    pt.raytrace_tiles([], 0, (WARM + STEPS) * SPP)
    img = pt.read_frame(B.FRAME_SAMPLE).astype(np.float64)
    pt.close()
    return img


@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_bench_line_and_dumped_outputs(tmp_path, single_render, full):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--workload", "c2",
           "--width", str(W), "--height", str(H), "--spp", str(SPP), "--steps", str(STEPS),
           "--warmup", str(WARM), "--dump-outputs", str(out)]
    if full:   # the CPU baselines have a time budget of their own (seconds): not in a test
        cmd += ["--full", "--no-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=REPO, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1                          # the result line alone goes to stdout
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == STEPS and line["warmup"] == WARM and line["full"] is full
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["kernel_ms"] > 0
    # value and ms_per_step state the same timed region (each rounded to 3 decimals; a step of
    # this size takes >= 0.05 ms, so the rounding of ms_per_step is within 1 %)
    assert line["value"] == pytest.approx(W * H * SPP / (line["ms_per_step"] * 1e-3) / 1e6, rel=2e-2)
    assert "cpu_baseline" not in line
    if full:
        assert line["roofline"]["counts_per_launch"]["samples"] == W * H * SPP
        assert line["parity"]["rmse"] < line["parity"]["tolerance"]
    else:
        assert "roofline" not in line and "parity" not in line
    assert sorted(os.listdir(out)) == ["sample_frame.npy"]
    frame = np.load(out / "sample_frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (H, W, 3) and np.isfinite(frame).all()
    rmse = float(np.sqrt(np.mean((frame.astype(np.float64) - single_render) ** 2)))
    print(f"dumped frame vs one render of the same samples: rmse {rmse:.3e}")
    assert rmse < 1e-6
