"""Timing of the time-optimisation entry points on BASELINE config 2's shape (4096 x 8 segments, r = 4) for docs/measurement_log.md:
(a) the cost + gradient launch next to the plain solve on the same batch, (b) one uavqp_time_optimize_device call at the default max_iters.
Warm-up, HIP events around the repeats, buffer sets rotated through more memory than the caches hold (as bench.py does).
The optimiser call updates its durations in place, so every repeat restores them first with a device copy (256 KB; inside the timed span).
    python tools/time_opt_bench.py [--reps 200] [--sets 64]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import uav_motion_planning_amd as U  # noqa: E402
from uav_motion_planning_amd import _lib, workloads as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--r", type=int, default=4)
    a = ap.parse_args()
    r, n, M = a.r, a.n, a.segments
    dev = torch.device("cuda", 0)
    b = W.uniform_batch(2, n, M, r, time_mode="distance")
    wp = torch.from_numpy(np.ascontiguousarray(b["waypoints"]).reshape(-1, 3)).to(dev)
    bc = torch.from_numpy(np.ascontiguousarray(b["bc"])).to(dev)
    T0 = torch.from_numpy(np.ascontiguousarray(b["times"]).ravel()).to(dev)
    sets = [dict(T=T0.clone(), coeff=torch.zeros(3 * 2 * r * n * M, dtype=torch.float64, device=dev), st=torch.zeros(n, dtype=torch.int32, device=dev),
                 cost=torch.zeros(n, dtype=torch.float64, device=dev), grad=torch.zeros(n * M, dtype=torch.float64, device=dev),
                 obj=torch.zeros((n, 2), dtype=torch.float64, device=dev), acc=torch.zeros(n, dtype=torch.int32, device=dev)) for _ in range(a.sets)]
    p = _lib.TimeOptParams()
    _lib.lib().uavqp_default_time_opt_params(ctypes.byref(p))
    out = dict(shape=f"{n} x {M} segments, r = {r}", reps=a.reps, buffer_sets=a.sets, max_iters=p.max_iters,
               rotated_megabytes=round(a.sets * sets[0]["coeff"].numel() * 8 / 2 ** 20, 1))
    with U.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)

        def solve(s):
            ctx.solve_batch_device(r, n, M, M, None, wp, s["T"], bc, s["coeff"], s["st"])

        def costgrad(s):
            ctx.cost_time_gradient_device(r, n, M, None, s["T"], s["coeff"], s["cost"], s["grad"])

        def optimise(s):
            s["T"].copy_(T0)
            ctx.time_optimize_device(r, n, M, M, n * M, None, wp, s["T"], bc, s["coeff"], s["st"], s["obj"], s["acc"])

        def timed(fn, reps):
            for i in range(min(a.sets, 16)):
                fn(sets[i % a.sets])
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(reps):
                fn(sets[i % a.sets])
            e1.record()
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1) * 1e3 / reps

        for s in sets:
            solve(s)
        out["solve_us"] = [round(timed(solve, a.reps), 2) for _ in range(3)]
        out["cost_gradient_us"] = [round(timed(costgrad, a.reps), 2) for _ in range(3)]
        out["time_optimize_us"] = [round(timed(optimise, a.reps), 1) for _ in range(3)]
        out["time_optimize_in_plain_solves"] = round(min(out["time_optimize_us"]) / min(out["solve_us"]), 1)
        s = sets[0]
        out["median_f_result_over_f_start"] = round(float(torch.median(s["obj"][:, 1] / s["obj"][:, 0])), 4)
        out["accepted_trials_median"] = int(torch.median(s["acc"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
