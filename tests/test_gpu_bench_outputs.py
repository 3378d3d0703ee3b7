"""-m gpu: a plain `bench.py --gpus 1 --steps K --warmup W` run -- the headline line alone, the K steps timed once -- and what
--dump-outputs writes: the last timed step's coefficients and status, the same numbers the C ABI gives for the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_its_dumped_outputs(tmp_path, gpu_ctx):
    import uav_motion_planning_amd as U
    from uav_motion_planning_amd import workloads as W
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(out_dir)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"{len(lines)} JSON lines on stdout"
    d = json.loads(lines[0])
    assert d["steps"] == 5 and d["warmup"] == 2 and d["timing"]["repeats"] == 1 and d["unit"] == "trajectories/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and abs(d["value"] - 4096 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["cpu_baseline"] is None and d["parity"] is None and not ({"other_configs", "time_modes", "pipelined", "kernels"} & set(d))
    coef, st = np.load(out_dir / "coeff.npy"), np.load(out_dir / "status.npy")
    assert coef.dtype == np.float64 and st.dtype == np.float64 and coef.size == 3 * 8 * 8 * 4096 and st.size == 4096
    assert np.all(st == U.UAVQP_SOLVED)
    b = W.uniform_batch(2, 4096, 8, 4, time_mode="distance", seed=W.SEED0 + 2)        # the batch bench.py builds for rank 0
    want, st_h = gpu_ctx.solve_batch_host(4, None, b["waypoints"], b["times"], b["bc"], uniform_segments=8)
    assert np.all(st_h == U.UAVQP_SOLVED)
    want = np.asarray(want).reshape(4096, -1)
    err = np.max(np.abs(coef.reshape(4096, -1) - want), axis=1) / np.max(np.abs(want), axis=1)
    assert err.max() < 1e-12, err.max()
