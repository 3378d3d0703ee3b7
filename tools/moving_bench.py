"""The measurements of the moving-obstacle penalty and its optimiser (docs/measurement_log.md).

    python tools/moving_bench.py [--reps 9] [--warmup 2] [--launches 200] [--trials 32]

1. Wall time per call of uavqp_moving_optimize_device beside uavqp_attitude_optimize_device on the same batch from the same start with the
   same attitude limits, the two ALTERNATING in the same run, at `--trials` trials: host clock around enqueue + stream synchronise, every
   call from the start copied into one of four rotating sets of buffers before the clock starts; medians and the spread.  The difference
   is what the moving-obstacle term costs: one launch per trial, and nothing else.
2. Device time of one moving-obstacle penalty launch (all six outputs) with 1 and with 8 obstacles per set beside one
   uavqp_limit_penalty_device launch on the same buffers: `--launches` launches between two events after a warm-up, inputs and outputs
   rotating through enough sets of buffers to exceed the 256 MB last-level cache.  Beside each, `*_host_enqueue_us`: the host's wall time per
   launch for enqueuing them (wrapper and C entry, before any synchronise) -- well under the device time, the figure is device-bound.

Shape: 4096 x 8 segments, r = 4 (config 2) in the 200 x 200 x 50 map of tools/waypoint_opt_bench.py.  Obstacles: every trajectory has a
set of its own of k one-segment tracks at constant velocity (about 1 m/s) that pass within 0.3 m of one of its interior waypoints at
the instant the start trajectory is there, under way for 0.4 of the flight -- so they wait, move and arrive inside the flight, and the
term is at work on every trajectory.  Flight and attitude limits as tools/attitude_opt_bench.py.  One JSON line per measurement.  Needs
the GPU: there is no CPU path."""
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


def line_tracks(wp, T, n, M, r, k, seed):
    """k one-segment tracks per trajectory -> the host arrays of a uavqp_moving_obstacles (uniform obstacle batch of 1 segment)"""
    rng = np.random.default_rng(seed)
    wp, T = wp.reshape(n, M + 1, 3), T.reshape(n, M)
    knots = np.concatenate([np.zeros((n, 1)), np.cumsum(T, axis=1)], axis=1)
    j = rng.integers(1, M, size=(n, k))
    p = np.take_along_axis(wp, j[:, :, None], axis=1) + rng.uniform(-0.3, 0.3, size=(n, k, 3)) * (1.0, 1.0, 0.3)
    Do = 0.4 * knots[:, -1:] * rng.uniform(0.9, 1.1, size=(n, k))
    ang = rng.uniform(0.0, 2.0 * np.pi, size=(n, k))
    vel = rng.uniform(0.7, 1.3, size=(n, k, 1)) * np.stack([np.cos(ang), np.sin(ang), rng.uniform(-0.1, 0.1, size=(n, k))], axis=-1)
    c = np.zeros((n, k, 3, 1, 2 * r))
    c[..., 0, 0] = p - 0.5 * Do[..., None] * vel
    c[..., 0, 1] = vel
    return dict(times=Do.ravel(), coeff=c.ravel(), start=(np.take_along_axis(knots, j, axis=1) - 0.5 * Do).ravel(),
                radius=rng.uniform(0.0, 0.2, size=n * k), set_offsets=np.arange(0, n * k + 1, k, dtype=np.int32),
                traj_set=np.arange(n, dtype=np.int32))


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
        T0 = np.asarray(b["times"], dtype=np.float64).ravel()
        total, nco = n * M, 3 * 2 * r * n * M
        d_bc, d_wp0, d_T0 = up(np.asarray(b["bc"], dtype=np.float64)), up(wp), up(T0)
        obstacles = {}
        for k in (1, 8):
            h = line_tracks(wp, T0, n, M, r, k, 900 + k)
            obstacles[k] = dict({key: up(v) for key, v in h.items()}, n_obs=n * k, uniform_segments=1, n_sets=n)

        def new_set():
            return dict(T=torch.empty_like(d_T0), wp=torch.empty_like(d_wp0), coeff=torch.zeros(nco, dtype=f64, device=dev),
                        status=torch.zeros(n, dtype=i32, device=dev), obj=torch.zeros((n, 2), dtype=f64, device=dev),
                        acc=torch.zeros(n, dtype=i32, device=dev), peak=torch.zeros((n, 2), dtype=f64, device=dev),
                        md=torch.zeros(n, dtype=f64, device=dev), out=torch.zeros(n, dtype=i32, device=dev),
                        apk=torch.zeros((n, 4), dtype=f64, device=dev), phi=torch.zeros(n, dtype=f64, device=dev),
                        g=torch.zeros(nco, dtype=f64, device=dev), gt=torch.zeros(total, dtype=f64, device=dev),
                        gs=torch.zeros(n, dtype=f64, device=dev), gap=torch.zeros(n, dtype=f64, device=dev),
                        near=torch.zeros(n, dtype=i32, device=dev))
        sets = [new_set() for _ in range(ROT)]
        s = sets[0]
        ctx.solve_batch_device(r, n, M, M, None, d_wp0, d_T0, d_bc, s["coeff"], s["status"])
        ctx.limit_penalty_device(r, n, M, None, d_T0, s["coeff"], status=s["status"], peak=s["peak"], v_max=1.0, a_max=1.0)
        ctx.attitude_penalty_device(r, n, M, None, d_T0, s["coeff"], status=s["status"], peak=s["apk"])
        ctx.synchronize()
        pk, apk = s["peak"].cpu().numpy(), s["apk"].cpu().numpy()
        lim = dict(v_max=0.7 * float(pk[:, 0].max()), a_max=0.7 * float(pk[:, 1].max()))
        mid = np.median(apk, axis=0)
        f_max = 0.7 * float(mid[0])
        att = dict(f_max=f_max, f_min=min(float(mid[1]) / 0.7, 0.9 * f_max), tilt_max=0.7 * min(float(mid[2]), 1.5), rate_max=0.7 * float(mid[3]))

        # ---- measurement 1: the two entries from the same start, alternating
        def entry(with_moving, k):
            s = sets[k % ROT]
            s["T"].copy_(d_T0)
            s["wp"].copy_(d_wp0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if with_moving:
                ctx.moving_optimize_device(r, n, M, M, total, None, s["wp"], s["T"], d_bc, m, obstacles[1], s["coeff"], s["status"], s["obj"],
                                           s["acc"], s["peak"], s["md"], s["out"], s["apk"], s["gap"], s["near"], limits=lim, attitude=att,
                                           max_iters=args.trials, max_move=move)
            else:
                ctx.attitude_optimize_device(r, n, M, M, total, None, s["wp"], s["T"], d_bc, m, s["coeff"], s["status"], s["obj"], s["acc"],
                                             s["peak"], s["md"], s["out"], s["apk"], limits=lim, attitude=att, max_iters=args.trials, max_move=move)
            ctx.synchronize()
            return time.perf_counter() - t0, s
        for k in range(args.warmup):
            entry(False, k)
            entry(True, k)
        t_parent, t_mov = [], []
        for k in range(args.reps):
            dt, s_parent = entry(False, 2 * k)
            t_parent.append(dt)
            f_parent = s_parent["obj"].cpu().numpy().copy()
            dt, s_mov = entry(True, 2 * k + 1)
            t_mov.append(dt)
        f_mov, gap1 = s_mov["obj"].cpu().numpy().copy(), s_mov["gap"].cpu().numpy().copy()
        ok = np.isfinite(f_mov[:, 0]) & np.isfinite(f_parent[:, 0])
        extra = statistics.median(t_mov) - statistics.median(t_parent)
        print(json.dumps(dict(measurement=1, shape=f"config2_{n}x{M}_r{r}", n_traj=n, segments=total, obstacles_per_set=1, max_iters=args.trials,
                              reps=args.reps, taking_part=int(ok.sum()), moving_ms=1e3 * statistics.median(t_mov), moving_ms_min=1e3 * min(t_mov),
                              moving_ms_max=1e3 * max(t_mov), attitude_ms=1e3 * statistics.median(t_parent), attitude_ms_min=1e3 * min(t_parent),
                              attitude_ms_max=1e3 * max(t_parent), ratio=statistics.median(t_mov) / statistics.median(t_parent),
                              extra_us_per_trial=1e6 * extra / (args.trials + 1),
                              median_f_start=float(np.median(f_mov[ok, 0])), median_f_result=float(np.median(f_mov[ok, 1])),
                              median_f_start_attitude=float(np.median(f_parent[ok, 0])), median_f_result_attitude=float(np.median(f_parent[ok, 1])),
                              median_min_gap_result=float(np.median(gap1[ok])))))

        # ---- measurement 2: one moving-obstacle penalty launch beside one limit penalty launch, at the start point
        one = 8 * (2 * nco + 2 * total) + 28 * n
        rot = max(ROT, min(64, -(-2 * CACHE_BYTES // one))) if one < CACHE_BYTES else ROT
        while len(sets) < rot:
            sets.append(new_set())
        ctx.solve_batch_device(r, n, M, M, None, d_wp0, d_T0, d_bc, sets[0]["coeff"], sets[0]["status"])   # (measurement 1 left its result there)
        for q in sets:
            q["coeff"].copy_(sets[0]["coeff"])
            q["status"].copy_(sets[0]["status"])
            q["T"].copy_(d_T0)
        penalised = {}
        for k in (1, 8):
            ctx.moving_penalty_device(r, n, M, None, d_T0, sets[0]["coeff"], obstacles[k], status=sets[0]["status"], penalty=sets[0]["phi"])
            ctx.synchronize()
            penalised[k] = int(np.count_nonzero(sets[0]["phi"].cpu().numpy() > 0))

        def moving(k):
            def fn(q):
                ctx.moving_penalty_device(r, n, M, None, q["T"], q["coeff"], obstacles[k], status=q["status"], penalty=q["phi"], grad_coeff=q["g"],
                                          grad_times=q["gt"], grad_start=q["gs"], min_gap=q["gap"], nearest=q["near"])
            return fn

        def limit(q):
            ctx.limit_penalty_device(r, n, M, None, q["T"], q["coeff"], status=q["status"], penalty=q["phi"], grad_coeff=q["g"], grad_times=q["gt"],
                                     peak=q["peak"], **lim)

        def timed(fn):
            for k in range(2 * rot):
                fn(sets[k % rot])
            torch.cuda.synchronize()
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            for k in range(args.launches):
                fn(sets[k % rot])
            host_us[fn].append(1e6 * (time.perf_counter() - t0) / args.launches)   # what the host took to ENQUEUE a launch
            b_.record()
            torch.cuda.synchronize()
            return 1e3 * a.elapsed_time(b_) / args.launches
        fns = (("moving_1", moving(1)), ("moving_8", moving(8)), ("limit", limit))
        host_us = {fn: [] for _, fn in fns}
        us = {name: [timed(fn) for _ in range(5)] for name, fn in fns}
        print(json.dumps(dict(measurement=2, shape=f"config2_{n}x{M}_r{r}", n_traj=n, segments=total, penalised_1=penalised[1],
                              penalised_8=penalised[8], launches=args.launches, buffer_sets=rot, bytes_per_set=one,
                              **{f"{k}_us": statistics.median(v) for k, v in us.items()}, **{f"{k}_us_min": min(v) for k, v in us.items()},
                              **{f"{k}_us_max": max(v) for k, v in us.items()},
                              **{f"{name}_host_enqueue_us": statistics.median(host_us[fn]) for name, fn in fns},
                              ratio_1_to_limit=statistics.median(us["moving_1"]) / statistics.median(us["limit"]),
                              ratio_8_to_limit=statistics.median(us["moving_8"]) / statistics.median(us["limit"]))))
        m.close()


if __name__ == "__main__":
    main()
