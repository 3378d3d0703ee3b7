"""Cost of ONE repair round of the corridor pipeline, rows repair against box repair, on the BASELINE config-5 batch (16384 ragged
kino-A*-like trajectories, M <= 24, r = 4, pillar cloud of 60 pillars at 0.2 m).  One round = (pipeline with repair_rounds = 1) -
(pipeline with repair_rounds = 0), medians of --reps wall-clock timings on one ctx after a warm-up call, fresh durations every call.
Prints one JSON line per mode with the collision counts.  Usage: python tools/pipeline_rows_repair_time.py [--reps 5] [--n 16384]."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import uav_motion_planning_amd as U  # noqa: E402
from uav_motion_planning_amd import workloads as W  # noqa: E402
from uav_motion_planning_amd.pipeline import corridor_pipeline_device  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--check-robot", type=float, nargs=2, default=None, help="check ellipsoid (r, h); default: the boxes' own")
    a = ap.parse_args()
    r, n, mx = 4, a.n, 24
    b = W.ragged_batch(5, n, r)
    so = b["seg_offsets"]
    wp = np.asarray(b["waypoints"]).reshape(-1, 3)
    obs = W.pillar_cloud(5, n_pillars=60, resolution=0.2)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_so, d_wp, d_bc, d_obs = up(so), up(wp), up(b["bc"]), up(obs)
    T0 = up(b["times"])
    kw = {} if a.check_robot is None else dict(check_robot=tuple(a.check_robot))
    with U.Context(0) as ctx:
        grid = ctx.obstacle_grid_build(d_obs, obs.shape[0], (a.check_robot[0] if a.check_robot else 0.4) + 0.1)

        def run(mode, rounds):
            d_T = T0.clone()
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = corridor_pipeline_device(ctx, r, d_so, d_wp, d_T, d_bc, d_obs, mx, repair_rounds=rounds, repair=mode, grid=grid, **kw)
            el = time.perf_counter() - t
            return el, res

        out = {}
        for mode in ("boxes", "rows"):
            run(mode, 1)
            t0 = [run(mode, 0)[0] for _ in range(a.reps)]
            t1, res = [], None
            for _ in range(a.reps):
                el, res = run(mode, 1)
                t1.append(el)
            rec = dict(mode=mode, n=n, pipeline_ms_0_rounds=1e3 * float(np.median(t0)), pipeline_ms_1_round=1e3 * float(np.median(t1)),
                       repair_round_ms=1e3 * float(np.median(t1) - np.median(t0)), colliding_before=res["colliding_before_repair"],
                       colliding_after=int((~res["collision_free"]).sum().item()), unsolved=int((res["status"] != U.UAVQP_SOLVED).sum().item()),
                       repair_rows=res.get("repair_rows", 0), check_robot=a.check_robot)
            out[mode] = rec
            print(json.dumps(rec), flush=True)
        ctx.obstacle_grid_destroy(grid)
    return out


if __name__ == "__main__":
    main()
