"""Device time of uavqp_swarm_optimize_device (docs/measurement_log.md), in the manner of tools/swarm_bench.py, beside
uavqp_spacetime_optimize_device on the same batch, and of the launches a trial is made of.

    python tools/swarm_opt_bench.py [--reps 7] [--warmup 3] [--launches 100] [--swarms 512] [--vehicles 8] [--segments 8] [--samples 64] [--iters 32]

Batch: that of tools/swarm_bench.py -- `--swarms` swarms of `--vehicles` vehicles of `--segments` segments, r = 4, laid by
tests/swarm_reference.py: scene() on a grid inside the 200 x 200 x 50 map of tools/waypoint_opt_bench.py, the swarm parameters of DESIGN.md
section 5.22 (the defaults, `--samples` clock samples).  Events around
  * one call of each optimiser with `--iters` trials and with 0 trials (waypoints and durations restored before every call, outside the
    events): ms per call, and us per trial = (t(iters) - t(0)) / iters;
  * `--launches` launches of each public entry a trial is made of, on the same batch: solve, flight penalty, plain swarm penalty
    (every gradient asked for), backward.  What is left of a trial after these is the step kernel -- for the swarm optimiser plus what the
    ACCUMULATING swarm penalty costs more than the plain one.
The accumulating instantiation and the two step kernels have no entry of their own: their times come from the kernel statistics of this
same run,
    tools/kstats.sh swarm_opt -- python tools/swarm_opt_bench.py --reps 2
which lists swarm_penalty_kernel<4, true> (the optimiser's) beside swarm_penalty_kernel<4, false> (the plain launches of this tool; the
optimiser is called without min_sep_out, so it launches none), and swarm_step_kernel beside spacetime_step_kernel.
One JSON line per measurement.  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uav_motion_planning_amd as U  # noqa: E402
from uav_motion_planning_amd import _lib  # noqa: E402
from uav_motion_planning_amd import workloads as W  # noqa: E402
from uav_motion_planning_amd.esdf import EsdfMap  # noqa: E402
import swarm_reference as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--swarms", type=int, default=512)
    ap.add_argument("--vehicles", type=int, default=8)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--iters", type=int, default=32)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/swarm_opt_bench.py needs the GPU: there is no CPU path")
    dev = torch.device("cuda", 0)
    f64, i32 = torch.float64, torch.int32
    version = _lib.lib().uavqp_version
    version.restype = ctypes.c_char_p
    print(json.dumps(dict(library=version().decode())))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    z = lambda k, t=f64: torch.zeros(k, dtype=t, device=dev)
    r, G, A, M, N = 4, args.swarms, args.vehicles, args.segments, args.samples
    n, total = G * A, G * A * M
    rng = np.random.default_rng(1)
    side = int(np.ceil(np.sqrt(G)))
    wps, Ts, starts = [], [], []
    for g in range(G):
        centre = (2.0 + 36.0 * ((g % side) + 0.5) / side, 2.0 + 36.0 * ((g // side) + 0.5) / side, 5.0)
        w, T, s = S.scene(rng, [M] * A, centre=centre, flight=0.1 * N * 0.8, start_span=(-0.05 * N * 0.1, 0.1 * N * 0.15))
        wps += w
        Ts += T
        starts.append(s)
    wp, T, start = np.concatenate(wps), np.concatenate(Ts), np.concatenate(starts)
    with U.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        cloud = W.pillar_cloud(5, n_pillars=60, resolution=0.2)
        cloud = cloud - cloud.min(axis=0) + 0.5
        esdf = EsdfMap(ctx, (200, 200, 50), (0.0, 0.0, 0.0), 0.2)
        esdf.set_cloud(up(cloud), inflation=0.2)
        esdf.update()
        wp0, T0, s0 = up(wp), up(T), up(start)
        d_wp, d_T, d_start = wp0.clone(), T0.clone(), s0.clone()
        d_bc = z(n * 2 * (r - 1) * 3)
        d_go = up((np.arange(G + 1) * A).astype(np.int32))
        coeff, status = z(3 * 2 * r * total), z(n, i32)
        obj_g, acc_g, obj_t, acc_t = z(2 * G), z(G, i32), z(2 * n), z(n, i32)
        sw = dict(n_samples=N)

        def restore():
            d_wp.copy_(wp0)
            d_T.copy_(T0)
            d_start.copy_(s0)

        def swarm_opt(iters):
            ctx.swarm_optimize_device(r, n, M, M, total, None, d_wp, d_T, d_bc, esdf, coeff, status, obj_g, n_groups=G, group_offsets=d_go,
                                      start=d_start, accepted_out=acc_g, swarm=sw, max_iters=iters)

        def spacetime_opt(iters):
            ctx.spacetime_optimize_device(r, n, M, M, total, None, d_wp, d_T, d_bc, esdf, coeff, status, obj_t, acc_t, max_iters=iters)

        calls = {"swarm_optimize": swarm_opt, "spacetime_optimize": spacetime_opt}
        ms = {(name, it): [] for name in calls for it in (args.iters, 0)}
        for rep in range(args.warmup + args.reps):
            for name, fn in calls.items():
                for it in (args.iters, 0):
                    restore()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    fn(it)
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ms[(name, it)].append(e0.elapsed_time(e1))
                    if name == "swarm_optimize" and it == args.iters and rep == 0:
                        o, a = obj_g.cpu().numpy().reshape(G, 2), acc_g.cpu().numpy()
                        print(json.dumps(dict(shape=dict(swarms=G, vehicles=A, segments=M, r=r, n_samples=N, trials=it),
                                              swarms_that_accepted=int(np.count_nonzero(a)), median_accepted=float(np.median(a)),
                                              median_f_ratio=float(np.median(o[:, 1] / o[:, 0])))))
        per_trial = {}
        for name in calls:
            full, none = statistics.median(ms[(name, args.iters)]), statistics.median(ms[(name, 0)])
            per_trial[name] = 1e3 * (full - none) / max(args.iters, 1)
            print(json.dumps(dict(entry=name, ms_per_call_median=round(full, 3), ms_min=round(min(ms[(name, args.iters)]), 3),
                                  ms_max=round(max(ms[(name, args.iters)]), 3), ms_with_0_trials=round(none, 3),
                                  us_per_trial=round(per_trial[name], 1), trials=args.iters, reps=args.reps)))

        # the public launches of a trial, on the start of the same batch
        restore()
        ctx.solve_batch_device(r, n, M, M, None, d_wp, d_T, d_bc, coeff, status)
        g_c, g_t, g_s, phi_g, phi_t, ms_v = z(3 * 2 * r * total), z(total), z(n), z(G), z(n), z(n)
        th_t, th_p = z(total), z(3 * (total + n))
        parts = {
            "solve": lambda: ctx.solve_batch_device(r, n, M, M, None, d_wp, d_T, d_bc, coeff, status),
            "flight_penalty": lambda: ctx.flight_penalty_device(r, n, M, None, d_T, coeff, esdf, status=status, penalty=phi_t, grad_coeff=g_c,
                                                                grad_times=g_t),
            "swarm_penalty_plain": lambda: ctx.swarm_penalty_device(r, n, M, None, d_T, coeff, n_groups=G, group_offsets=d_go, start=d_start,
                                                                    status=status, penalty=phi_g, grad_coeff=g_c, grad_times=g_t, grad_start=g_s,
                                                                    **sw),
            "backward": lambda: ctx.solve_backward_device(r, n, M, M, total, None, d_wp, d_T, d_bc, coeff, g_c, grad_times=th_t,
                                                          grad_waypoints=th_p, status=status),
        }
        us = {}
        for name, fn in parts.items():
            t = []
            for rep in range(args.warmup + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    t.append(1e3 * e0.elapsed_time(e1) / args.launches)
            us[name] = statistics.median(t)
            print(json.dumps(dict(launch=name, us_per_launch_median=round(us[name], 2), us_min=round(min(t), 2), us_max=round(max(t), 2),
                                  reps=args.reps, launches=args.launches)))
        common = us["solve"] + us["flight_penalty"] + us["backward"]
        print(json.dumps(dict(per_trial_us=dict(
            swarm_optimize=round(per_trial["swarm_optimize"], 1), spacetime_optimize=round(per_trial["spacetime_optimize"], 1),
            solve_plus_flight_plus_backward=round(common, 1),
            spacetime_step_by_difference=round(per_trial["spacetime_optimize"] - common, 1),
            swarm_step_plus_accumulate_extra_by_difference=round(per_trial["swarm_optimize"] - common - us["swarm_penalty_plain"], 1)))))
        esdf.close()


if __name__ == "__main__":
    main()
