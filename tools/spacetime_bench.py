"""The two measurements of the joint waypoint / duration optimiser (docs/measurement_log.md).

    python tools/spacetime_bench.py [--reps 9] [--warmup 2] [--launches 200] [--shape NAME]

1. Wall time per call of uavqp_spacetime_optimize_device at the default max_iters beside ALTERNATING uavqp_time_optimize_limits_device and
   uavqp_waypoint_optimize_device with the same total number of inner solves (a call with k trials solves k + 2 times: 32 trials of the joint
   optimiser = 34 solves = 2 rounds of { 7 duration trials, 6 waypoint trials }), and the final f of both UNDER THE JOINT OBJECTIVE (a joint
   call with max_iters = 0 at the alternation's result evaluates it).  Host clock around enqueue + stream synchronise, every call from the
   same start copied into one of four rotating sets of buffers before the clock starts; medians and the spread.
2. Device time of one fused penalty launch beside the two separate penalty launches: `--launches` launches between two events after a
   warm-up, inputs and outputs rotating through enough sets of buffers to exceed the 256 MB last-level cache where one set is smaller.

3. `--method lbfgs` (instead of 1 and 2): uavqp_spacetime_lbfgs_device beside uavqp_spacetime_optimize_device from the
   same start, alternating in the same run, at 32 and at 256 trials: wall time per call of both and the median final joint objective of
   both, next to the hand alternation's at 34 solves (as in 1) -- the comparison recorded in DESIGN.md section 5.20 as 4264 / 832 and
   1062 / 696.  Under `rocprofv3 --kernel-trace --stats` the same run gives the time of spacetime_lbfgs_step_kernel.

Shapes: 4096 x 8 segments, r = 4 (config 2) in the 200 x 200 x 50 map of tools/waypoint_opt_bench.py, and the ragged 14-trajectory batch of
tests/test_gpu_spacetime.py (r = 4) in its own scene.  Limits: 0.7 x the batch's sampled peak at the start for config 2, the test's own for
the test batch.  One JSON line per shape and measurement.  Needs the GPU: there is no CPU path."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import uav_motion_planning_amd as U  # noqa: E402
from uav_motion_planning_amd import _lib  # noqa: E402
from uav_motion_planning_amd import workloads as W  # noqa: E402
from uav_motion_planning_amd.esdf import EsdfMap  # noqa: E402
from waypoint_opt_bench import into_map  # noqa: E402

ROT = 4
ROUNDS, IT_T, IT_W = 2, 7, 6
CACHE_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--method", choices=("gd", "lbfgs"), default="gd", help="lbfgs: measurement 3 alone")
    ap.add_argument("--trials", type=int, nargs="+", default=[32, 256], help="max_iters of measurement 3")
    args = ap.parse_args()
    import torch
    import spacetime_reference as R
    import waypoint_opt_reference as WR
    dev = torch.device("cuda", 0)
    f64, i32 = torch.float64, torch.int32
    pp = _lib.SpacetimeParams()
    _lib.lib().uavqp_default_spacetime_params(ctypes.byref(pp))
    iters = pp.max_iters
    assert iters + 2 == ROUNDS * (IT_T + 2 + IT_W + 2), "the alternation no longer has the joint call's number of solves"
    version = _lib.lib().uavqp_version
    version.restype = ctypes.c_char_p
    print(json.dumps(dict(library=version().decode())))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    with U.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        cloud = W.pillar_cloud(5, n_pillars=60, resolution=0.2)
        lo = cloud.min(axis=0) - 0.5
        big = EsdfMap(ctx, (200, 200, 50), tuple(lo), 0.2)
        big.set_cloud(up(cloud), inflation=0.2)
        big.update()
        sc = R.scene()
        small = EsdfMap(ctx, WR.DIMS, WR.ORIGIN, WR.RES, WR.MAX_DIST)
        small.set_occupancy(sc["occ"])
        small.update()
        ctx.synchronize()
        hi = lo + np.array(big.dims) * big.resolution
        b2 = W.uniform_batch(2, 4096, 8, 4, time_mode="distance")
        b2 = dict(b2, waypoints=into_map(np.ascontiguousarray(b2["waypoints"], dtype=np.float64).reshape(-1, 3), lo, hi))
        shapes = {"config2_4096x8_r4": (b2, 8, big, None, 2.0), "test_batch_14_r4": (R.cases(4), 0, small, R.LIMITS_OF[4], R.PARAMS["max_move"])}
        for name, (b, uni, m, lim, move) in shapes.items():
            if args.shape and name != args.shape:
                continue
            r = b["r"]
            so = np.ascontiguousarray(b["seg_offsets"], dtype=np.int32)
            n, total, mmax = so.size - 1, int(so[-1]), int(np.max(np.diff(so)))
            d_so, d_bc = up(so), up(np.asarray(b["bc"], dtype=np.float64))
            d_wp0, d_T0 = up(np.asarray(b["waypoints"], dtype=np.float64).reshape(-1, 3)), up(np.asarray(b["times"], dtype=np.float64).ravel())
            nco = 3 * 2 * r * total

            def new_set():
                return dict(T=torch.empty_like(d_T0), wp=torch.empty_like(d_wp0), coeff=torch.zeros(nco, dtype=f64, device=dev),
                            status=torch.zeros(n, dtype=i32, device=dev), obj=torch.zeros((n, 2), dtype=f64, device=dev),
                            acc=torch.zeros(n, dtype=i32, device=dev), peak=torch.zeros((n, 2), dtype=f64, device=dev),
                            md=torch.zeros(n, dtype=f64, device=dev), out=torch.zeros(n, dtype=i32, device=dev),
                            phi=torch.zeros(n, dtype=f64, device=dev), phi2=torch.zeros(n, dtype=f64, device=dev),
                            g=torch.zeros(nco, dtype=f64, device=dev), g2=torch.zeros(nco, dtype=f64, device=dev),
                            gt=torch.zeros(total, dtype=f64, device=dev), gt2=torch.zeros(total, dtype=f64, device=dev))
            sets = [new_set() for _ in range(ROT)]
            s = sets[0]
            ctx.solve_batch_device(r, n, uni, mmax, d_so, d_wp0, d_T0, d_bc, s["coeff"], s["status"])
            if lim is None:
                ctx.limit_penalty_device(r, n, uni, d_so, d_T0, s["coeff"], status=s["status"], peak=s["peak"], v_max=1.0, a_max=1.0)
                ctx.synchronize()
                pk = s["peak"].cpu().numpy()
                lim = dict(v_max=0.7 * float(pk[:, 0].max()), a_max=0.7 * float(pk[:, 1].max()))
            ctx.synchronize()

            def joint(s, max_iters):
                ctx.spacetime_optimize_device(r, n, uni, mmax, total, d_so, s["wp"], s["T"], d_bc, m, s["coeff"], s["status"], s["obj"], s["acc"],
                                              s["peak"], s["md"], s["out"], limits=lim, max_iters=max_iters, max_move=move)

            def call(jointly, k):
                s = sets[k % ROT]
                s["T"].copy_(d_T0)
                s["wp"].copy_(d_wp0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if jointly:
                    joint(s, iters)
                else:
                    for _ in range(ROUNDS):
                        ctx.time_optimize_limits_device(r, n, uni, mmax, total, d_so, s["wp"], s["T"], d_bc, s["coeff"], s["status"], s["obj"],
                                                        s["acc"], limits=lim, max_iters=IT_T)
                        # (the waypoint optimiser's box is around ITS start: the second round's box is centred on the first round's result)
                        ctx.waypoint_optimize_device(r, n, uni, mmax, total, d_so, s["wp"], s["T"], d_bc, m, s["coeff"], s["status"], s["obj"],
                                                     s["acc"], max_iters=IT_W, max_move=move / ROUNDS)
                ctx.synchronize()
                return time.perf_counter() - t0, s

            if args.method == "lbfgs":
                # ---- measurement 3: the two joint entries from the same start, alternating; the hand alternation once for its objective
                def entry(lbfgs, k, max_iters):
                    s = sets[k % ROT]
                    s["T"].copy_(d_T0)
                    s["wp"].copy_(d_wp0)
                    torch.cuda.synchronize()
                    fn = ctx.spacetime_lbfgs_device if lbfgs else ctx.spacetime_optimize_device
                    t0 = time.perf_counter()
                    fn(r, n, uni, mmax, total, d_so, s["wp"], s["T"], d_bc, m, s["coeff"], s["status"], s["obj"], s["acc"], s["peak"], s["md"],
                       s["out"], limits=lim, max_iters=max_iters, max_move=move)
                    ctx.synchronize()
                    return time.perf_counter() - t0, s
                _, s_alt = call(False, 0)
                joint(s_alt, 0)                               # the joint objective at the alternation's result
                ctx.synchronize()
                f_alt = s_alt["obj"].cpu().numpy().copy()
                for trials in args.trials:
                    reps = args.reps if trials <= 64 else max(3, args.reps // 3)
                    for k in range(args.warmup):
                        entry(False, k, trials)
                        entry(True, k, trials)
                    t_gd, t_qn = [], []
                    for k in range(reps):
                        dt, s_gd = entry(False, 2 * k, trials)
                        t_gd.append(dt)
                        f_gd, acc_gd = s_gd["obj"].cpu().numpy().copy(), s_gd["acc"].cpu().numpy().copy()
                        dt, s_qn = entry(True, 2 * k + 1, trials)
                        t_qn.append(dt)
                    f_qn, acc_qn = s_qn["obj"].cpu().numpy().copy(), s_qn["acc"].cpu().numpy().copy()
                    ok = np.isfinite(f_gd[:, 0]) & np.isfinite(f_qn[:, 0]) & np.isfinite(f_alt[:, 0])
                    print(json.dumps(dict(measurement=3, shape=name, n_traj=n, segments=total, max_iters=trials, reps=reps, taking_part=int(ok.sum()),
                                          lbfgs_ms=1e3 * statistics.median(t_qn), lbfgs_ms_min=1e3 * min(t_qn), lbfgs_ms_max=1e3 * max(t_qn),
                                          gradient_ms=1e3 * statistics.median(t_gd), gradient_ms_min=1e3 * min(t_gd), gradient_ms_max=1e3 * max(t_gd),
                                          ratio=statistics.median(t_qn) / statistics.median(t_gd),
                                          median_f_start=float(np.median(f_qn[ok, 0])), median_f_lbfgs=float(np.median(f_qn[ok, 1])),
                                          median_f_gradient=float(np.median(f_gd[ok, 1])),
                                          median_f_alternating_34_solves=float(np.median(f_alt[ok, 0])),
                                          lbfgs_lower_than_gradient_in=int(np.count_nonzero(f_qn[ok, 1] < f_gd[ok, 1])),
                                          lbfgs_lower_than_alternating_in=int(np.count_nonzero(f_qn[ok, 1] < f_alt[ok, 0])),
                                          median_accepted_lbfgs=float(np.median(acc_qn[ok])), median_accepted_gradient=float(np.median(acc_gd[ok])),
                                          lbfgs_peak_v_a_max=[float(x) for x in s_qn["peak"].cpu().numpy()[ok].max(axis=0)],
                                          lbfgs_min_dist_min=float(s_qn["md"].cpu().numpy()[ok].min()))))
                continue
            for k in range(args.warmup):
                call(False, k)
                call(True, k)
            t_alt, t_joint = [], []
            for k in range(args.reps):
                t_alt.append(call(False, 2 * k)[0])
                dt, s_joint = call(True, 2 * k + 1)
                t_joint.append(dt)
            f_joint = s_joint["obj"].cpu().numpy().copy()
            peak_j, md_j = s_joint["peak"].cpu().numpy().copy(), s_joint["md"].cpu().numpy().copy()
            _, s_alt = call(False, 0)
            joint(s_alt, 0)                                   # the joint objective at the alternation's result
            ctx.synchronize()
            f_alt = s_alt["obj"].cpu().numpy()
            ok = np.isfinite(f_joint[:, 0]) & np.isfinite(f_alt[:, 0])
            print(json.dumps(dict(measurement=1, shape=name, n_traj=n, segments=total, max_iters=iters, solves=iters + 2,
                                  alternation=f"{ROUNDS} x ({IT_T} duration + {IT_W} waypoint trials)",
                                  joint_ms=1e3 * statistics.median(t_joint), joint_ms_min=1e3 * min(t_joint), joint_ms_max=1e3 * max(t_joint),
                                  alternating_ms=1e3 * statistics.median(t_alt), alternating_ms_min=1e3 * min(t_alt), alternating_ms_max=1e3 * max(t_alt),
                                  ratio=statistics.median(t_joint) / statistics.median(t_alt), taking_part=int(ok.sum()),
                                  median_f_start=float(np.median(f_joint[ok, 0])), median_f_joint=float(np.median(f_joint[ok, 1])),
                                  median_f_alternating=float(np.median(f_alt[ok, 0])),
                                  joint_lower_in=int(np.count_nonzero(f_joint[ok, 1] < f_alt[ok, 0])),
                                  joint_peak_v_a_max=[float(x) for x in peak_j[ok].max(axis=0)], joint_min_dist_min=float(md_j[ok].min()),
                                  alternating_peak_v_a_max=[float(x) for x in s_alt["peak"].cpu().numpy()[ok].max(axis=0)],
                                  alternating_min_dist_min=float(s_alt["md"].cpu().numpy()[ok].min()))))

            # ---- measurement 2: one fused launch against the two separate launches, at the start point
            one = 8 * (2 * nco + 2 * total) + 12 * n
            rot = max(ROT, min(64, -(-2 * CACHE_BYTES // one))) if one < CACHE_BYTES else ROT
            while len(sets) < rot:
                sets.append(new_set())
            for q in sets:
                q["coeff"].copy_(sets[0]["coeff"])
                q["status"].copy_(sets[0]["status"])
                q["T"].copy_(d_T0)

            def fused(q):
                ctx.flight_penalty_device(r, n, uni, d_so, q["T"], q["coeff"], m, status=q["status"], penalty=q["phi"], grad_coeff=q["g"],
                                          grad_times=q["gt"], limits=lim)

            def separate(q):
                ctx.limit_penalty_device(r, n, uni, d_so, q["T"], q["coeff"], status=q["status"], penalty=q["phi"], grad_coeff=q["g"],
                                         grad_times=q["gt"], **lim)
                ctx.clearance_penalty_device(r, n, uni, d_so, q["T"], q["coeff"], m, status=q["status"], penalty=q["phi2"], grad_coeff=q["g2"],
                                             grad_times=q["gt2"])

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
            us_f = [timed(fused) for _ in range(5)]
            us_s = [timed(separate) for _ in range(5)]
            print(json.dumps(dict(measurement=2, shape=name, n_traj=n, segments=total, launches=args.launches, buffer_sets=rot,
                                  bytes_per_set=one, fused_us=statistics.median(us_f), fused_us_min=min(us_f), fused_us_max=max(us_f),
                                  separate_us=statistics.median(us_s), separate_us_min=min(us_s), separate_us_max=max(us_s),
                                  ratio=statistics.median(us_f) / statistics.median(us_s))))
        big.close()
        small.close()


if __name__ == "__main__":
    main()
