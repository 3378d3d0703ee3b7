"""The measurements of the attitude penalty and its optimiser (docs/measurement_log.md).

    python tools/attitude_opt_bench.py [--reps 9] [--warmup 2] [--launches 200] [--trials 32]

1. Wall time per call of uavqp_attitude_optimize_device beside uavqp_spacetime_lbfgs_device on the same batch from the same start, the two
   ALTERNATING in the same run, at `--trials` trials: host clock around enqueue + stream synchronise, every call from the start copied
   into one of four rotating sets of buffers before the clock starts; medians and the spread.  The difference is what the attitude term
   costs: one launch per trial.
2. Device time of one attitude penalty launch (all four outputs; and the penalty and the two gradients without the peaks, which is what
   the optimiser's loop pays apart from the read-modify-write) beside one uavqp_limit_penalty_device launch on the same buffers:
   `--launches` launches between two events after a warm-up, inputs and outputs rotating through enough sets of buffers to exceed the 256 MB
   last-level cache.  Under `rocprofv3 --kernel-trace --stats` the same run gives the time of attitude_penalty_kernel inside the optimiser.

Shape: 4096 x 8 segments, r = 4 (config 2) in the 200 x 200 x 50 map of tools/waypoint_opt_bench.py.  Limits: 0.7 x the batch's sampled peaks
at the start for the flight limits (as tools/spacetime_bench.py), 0.7 x the median of the per-trajectory peaks for the attitude limits.  One JSON line per measurement.  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import uav_motion_planning_amd as U  # noqa: E402
from uav_motion_planning_amd import _lib  # noqa: E402
from uav_motion_planning_amd import workloads as W  # noqa: E402
from uav_motion_planning_amd.esdf import EsdfMap  # noqa: E402
from waypoint_opt_bench import into_map  # noqa: E402

ROT = 4
CACHE_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--trials", type=int, default=32)
    ap.add_argument("--n-traj", type=int, default=4096)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    f64, i32 = torch.float64, torch.int32
    version = _lib.lib().uavqp_version
    version.restype = ctypes.c_char_p
    print(json.dumps(dict(library=version().decode())))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    with U.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        cloud = W.pillar_cloud(5, n_pillars=60, resolution=0.2)
        lo = cloud.min(axis=0) - 0.5
        m = EsdfMap(ctx, (200, 200, 50), tuple(lo), 0.2)
        m.set_cloud(up(cloud), inflation=0.2)
        m.update()
        ctx.synchronize()
        hi = lo + np.array(m.dims) * m.resolution
        r, M, n, move = 4, 8, args.n_traj, 2.0
        b = W.uniform_batch(2, n, M, r, time_mode="distance")
        wp = into_map(np.ascontiguousarray(b["waypoints"], dtype=np.float64).reshape(-1, 3), lo, hi)
        total, nco = n * M, 3 * 2 * r * n * M
        d_bc, d_wp0, d_T0 = up(np.asarray(b["bc"], dtype=np.float64)), up(wp), up(np.asarray(b["times"], dtype=np.float64).ravel())

        def new_set():
            return dict(T=torch.empty_like(d_T0), wp=torch.empty_like(d_wp0), coeff=torch.zeros(nco, dtype=f64, device=dev),
                        status=torch.zeros(n, dtype=i32, device=dev), obj=torch.zeros((n, 2), dtype=f64, device=dev),
                        acc=torch.zeros(n, dtype=i32, device=dev), peak=torch.zeros((n, 2), dtype=f64, device=dev),
                        md=torch.zeros(n, dtype=f64, device=dev), out=torch.zeros(n, dtype=i32, device=dev),
                        apk=torch.zeros((n, 4), dtype=f64, device=dev), phi=torch.zeros(n, dtype=f64, device=dev),
                        g=torch.zeros(nco, dtype=f64, device=dev), gt=torch.zeros(total, dtype=f64, device=dev))
        sets = [new_set() for _ in range(ROT)]
        s = sets[0]
        ctx.solve_batch_device(r, n, M, M, None, d_wp0, d_T0, d_bc, s["coeff"], s["status"])
        ctx.limit_penalty_device(r, n, M, None, d_T0, s["coeff"], status=s["status"], peak=s["peak"], v_max=1.0, a_max=1.0)
        ctx.attitude_penalty_device(r, n, M, None, d_T0, s["coeff"], status=s["status"], peak=s["apk"])
        ctx.synchronize()
        pk, apk = s["peak"].cpu().numpy(), s["apk"].cpu().numpy()
        lim = dict(v_max=0.7 * float(pk[:, 0].max()), a_max=0.7 * float(pk[:, 1].max()))
        # (the MEDIAN of the per-trajectory peaks: the start's body rates have a long tail, and a limit at 0.7 x the largest binds on a handful)
        mid = np.median(apk, axis=0)
        f_max = 0.7 * float(mid[0])
        att = dict(f_max=f_max, f_min=min(float(mid[1]) / 0.7, 0.9 * f_max), tilt_max=0.7 * min(float(mid[2]), 1.5), rate_max=0.7 * float(mid[3]))

        # ---- measurement 1: the two entries from the same start, alternating
        def entry(with_attitude, k):
            s = sets[k % ROT]
            s["T"].copy_(d_T0)
            s["wp"].copy_(d_wp0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if with_attitude:
                ctx.attitude_optimize_device(r, n, M, M, total, None, s["wp"], s["T"], d_bc, m, s["coeff"], s["status"], s["obj"], s["acc"],
                                             s["peak"], s["md"], s["out"], s["apk"], limits=lim, attitude=att, max_iters=args.trials, max_move=move)
            else:
                ctx.spacetime_lbfgs_device(r, n, M, M, total, None, s["wp"], s["T"], d_bc, m, s["coeff"], s["status"], s["obj"], s["acc"],
                                           s["peak"], s["md"], s["out"], limits=lim, max_iters=args.trials, max_move=move)
            ctx.synchronize()
            return time.perf_counter() - t0, s
        for k in range(args.warmup):
            entry(False, k)
            entry(True, k)
        t_plain, t_att = [], []
        for k in range(args.reps):
            dt, s_plain = entry(False, 2 * k)
            t_plain.append(dt)
            f_plain = s_plain["obj"].cpu().numpy().copy()
            dt, s_att = entry(True, 2 * k + 1)
            t_att.append(dt)
        f_att, apk1 = s_att["obj"].cpu().numpy().copy(), s_att["apk"].cpu().numpy().copy()
        ok = np.isfinite(f_att[:, 0]) & np.isfinite(f_plain[:, 0])
        extra = statistics.median(t_att) - statistics.median(t_plain)
        print(json.dumps(dict(measurement=1, shape=f"config2_{n}x{M}_r{r}", n_traj=n, segments=total, max_iters=args.trials, reps=args.reps,
                              taking_part=int(ok.sum()), attitude_ms=1e3 * statistics.median(t_att), attitude_ms_min=1e3 * min(t_att),
                              attitude_ms_max=1e3 * max(t_att), lbfgs_ms=1e3 * statistics.median(t_plain), lbfgs_ms_min=1e3 * min(t_plain),
                              lbfgs_ms_max=1e3 * max(t_plain), ratio=statistics.median(t_att) / statistics.median(t_plain),
                              extra_us_per_trial=1e6 * extra / (args.trials + 1), attitude_limits=att,
                              median_f_start=float(np.median(f_att[ok, 0])), median_f_result=float(np.median(f_att[ok, 1])),
                              median_f_start_lbfgs=float(np.median(f_plain[ok, 0])), median_f_result_lbfgs=float(np.median(f_plain[ok, 1])),
                              attitude_peak_start_max=[float(x) for x in apk[ok].max(axis=0)],
                              attitude_peak_result_max=[float(x) for x in apk1[ok].max(axis=0)])))

        # ---- measurement 2: one attitude penalty launch beside one limit penalty launch, at the start point
        one = 8 * (2 * nco + 2 * total) + 12 * n
        rot = max(ROT, min(64, -(-2 * CACHE_BYTES // one))) if one < CACHE_BYTES else ROT
        while len(sets) < rot:
            sets.append(new_set())
        ctx.solve_batch_device(r, n, M, M, None, d_wp0, d_T0, d_bc, sets[0]["coeff"], sets[0]["status"])   # (measurement 1 left its result there)
        for q in sets:
            q["coeff"].copy_(sets[0]["coeff"])
            q["status"].copy_(sets[0]["status"])
            q["T"].copy_(d_T0)
        ctx.attitude_penalty_device(r, n, M, None, d_T0, sets[0]["coeff"], status=sets[0]["status"], penalty=sets[0]["phi"], **att)
        ctx.synchronize()
        penalised = int(np.count_nonzero(sets[0]["phi"].cpu().numpy() > 0))

        def attitude_all(q):
            ctx.attitude_penalty_device(r, n, M, None, q["T"], q["coeff"], status=q["status"], penalty=q["phi"], grad_coeff=q["g"],
                                        grad_times=q["gt"], peak=q["apk"], **att)

        def attitude_no_peak(q):
            ctx.attitude_penalty_device(r, n, M, None, q["T"], q["coeff"], status=q["status"], penalty=q["phi"], grad_coeff=q["g"],
                                        grad_times=q["gt"], **att)

        def limit(q):
            ctx.limit_penalty_device(r, n, M, None, q["T"], q["coeff"], status=q["status"], penalty=q["phi"], grad_coeff=q["g"], grad_times=q["gt"],
                                     peak=q["peak"], **lim)

        def timed(fn):
            for k in range(2 * rot):
                fn(sets[k % rot])
            torch.cuda.synchronize()
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(args.launches):
                fn(sets[k % rot])
            b_.record()
            torch.cuda.synchronize()
            return 1e3 * a.elapsed_time(b_) / args.launches
        us = {name: [timed(fn) for _ in range(5)] for name, fn in (("attitude", attitude_all), ("attitude_no_peak", attitude_no_peak),
                                                                   ("limit", limit))}
        print(json.dumps(dict(measurement=2, shape=f"config2_{n}x{M}_r{r}", n_traj=n, segments=total, penalised=penalised, launches=args.launches,
                              buffer_sets=rot, bytes_per_set=one,
                              **{f"{k}_us": statistics.median(v) for k, v in us.items()}, **{f"{k}_us_min": min(v) for k, v in us.items()},
                              **{f"{k}_us_max": max(v) for k, v in us.items()},
                              ratio_to_limit=statistics.median(us["attitude"]) / statistics.median(us["limit"]))))
        m.close()


if __name__ == "__main__":
    main()
