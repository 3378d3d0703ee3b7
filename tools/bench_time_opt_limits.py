"""Wall time per call of the limit-aware duration optimiser against the plain one at the same max_iters.

    python tools/bench_time_opt_limits.py [--reps 15] [--warmup 3] [--max-iters 24] [--once]

Shapes: 4096 x 8 segments, r = 4 (config 2) and the 32768-trajectory ragged config-4 shape (M in [4, 24], r = 4).  Limits: 0.7 x the batch's
sampled peak at the start, default weights.  The two optimisers alternate inside one loop; every call starts from the same durations,
copied into one of four rotating sets of buffers before the clock starts; a call is timed by the host clock around enqueue + stream
synchronise; medians and the spread (min .. max) are printed, one JSON line per shape at the end.  --once runs each optimiser a single
time per shape with no timing: the run to put under `rocprofv3 --kernel-trace --stats` for the per-kernel shares.
Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uav_motion_planning_amd as U  # noqa: E402
from uav_motion_planning_amd import workloads as W  # noqa: E402

ROT = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-iters", type=int, default=24)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    shapes = {
        "config2_4096x8_r4": (W.uniform_batch(2, 4096, 8, 4, time_mode="distance"), 8),
        "config4_ragged_32768_r4": (W.ragged_batch(4, 32768, 4), 0),
    }
    results = []
    with U.Context(0) as ctx:
        for name, (b, uni) in shapes.items():
            r = b["r"]
            so = np.ascontiguousarray(b["seg_offsets"], dtype=np.int32)
            n, total, mmax = so.size - 1, int(so[-1]), int(np.max(np.diff(so)))
            d_so = torch.from_numpy(so).to(dev)
            d_wp = torch.from_numpy(np.ascontiguousarray(b["waypoints"], dtype=np.float64).reshape(-1, 3)).to(dev)
            d_bc = torch.from_numpy(np.ascontiguousarray(b["bc"], dtype=np.float64)).to(dev)
            d_T0 = torch.from_numpy(np.ascontiguousarray(b["times"], dtype=np.float64).ravel()).to(dev)
            sets = [dict(T=torch.empty_like(d_T0), coeff=torch.zeros(3 * 2 * r * total, dtype=torch.float64, device=dev),
                         status=torch.zeros(n, dtype=torch.int32, device=dev), obj=torch.zeros((n, 2), dtype=torch.float64, device=dev),
                         acc=torch.zeros(n, dtype=torch.int32, device=dev), peak=torch.zeros((n, 2), dtype=torch.float64, device=dev))
                    for _ in range(ROT)]
            # limits from the start's own peaks
            s = sets[0]
            ctx.solve_batch_device(r, n, uni, mmax, d_so, d_wp, d_T0, d_bc, s["coeff"], s["status"])
            ctx.limit_penalty_device(r, n, uni, d_so, d_T0, s["coeff"], status=s["status"], peak=s["peak"], v_max=1.0, a_max=1.0)
            ctx.synchronize()
            pk = s["peak"].cpu().numpy()
            lim = dict(v_max=0.7 * float(pk[:, 0].max()), a_max=0.7 * float(pk[:, 1].max()))

            def call(limited, k):
                s = sets[k % ROT]
                s["T"].copy_(d_T0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if limited:
                    ctx.time_optimize_limits_device(r, n, uni, mmax, total, d_so, d_wp, s["T"], d_bc, s["coeff"], s["status"], s["obj"], s["acc"],
                                                    peak_out=s["peak"], limits=lim, max_iters=args.max_iters)
                else:
                    ctx.time_optimize_device(r, n, uni, mmax, total, d_so, d_wp, s["T"], d_bc, s["coeff"], s["status"], s["obj"], s["acc"],
                                             max_iters=args.max_iters)
                ctx.synchronize()
                return time.perf_counter() - t0

            if args.once:
                call(False, 0)
                call(True, 1)
                continue
            for k in range(args.warmup):
                call(False, k)
                call(True, k)
            t_plain, t_lim = [], []
            for k in range(args.reps):
                t_plain.append(call(False, 2 * k))
                t_lim.append(call(True, 2 * k + 1))
            s = sets[(2 * args.reps - 1) % ROT]
            obj, pk1 = s["obj"].cpu().numpy(), s["peak"].cpu().numpy()
            ok = np.isfinite(obj[:, 0])
            res = dict(shape=name, n_traj=n, segments=total, max_iters=args.max_iters, v_max=lim["v_max"], a_max=lim["a_max"],
                       plain_ms=1e3 * statistics.median(t_plain), plain_ms_min=1e3 * min(t_plain), plain_ms_max=1e3 * max(t_plain),
                       limits_ms=1e3 * statistics.median(t_lim), limits_ms_min=1e3 * min(t_lim), limits_ms_max=1e3 * max(t_lim),
                       ratio=statistics.median(t_lim) / statistics.median(t_plain),
                       violating_at_start=int(np.count_nonzero((pk[ok] > 0.7 * pk.max(axis=0)).any(axis=1))),
                       violating_at_result=int(np.count_nonzero((pk1[ok] > 1.0).any(axis=1))), worst_peak_at_result=float(pk1[ok].max()))
            results.append(res)
    for res in results:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
