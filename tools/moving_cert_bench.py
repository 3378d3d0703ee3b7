"""The measurements of the certificate against moving-obstacle tracks (docs/measurement_log.md).

    python tools/moving_cert_bench.py [--launches 50] [--runs 5] [--n-traj 4096]

Device time of one uavqp_moving_certificate_device launch (all five outputs) at depth 3 and 5 with 1 and with 8 obstacles per set, beside
the yardstick: what include/uavqp.h recommended before this entry existed, uavqp_separation_certificate_device on `n_traj` groups of one
vehicle plus its 8 tracks (a batch of 9 n_traj trajectories), with a clock window that covers the same flight in the same number of leaves
per vehicle (n_cells = M cells of the longest flight / M, the same depth).  `--launches` launches between two events after a warm-up,
inputs and outputs rotating through enough sets of buffers to exceed the 256 MB last-level cache; `--runs` such runs, median and spread.
Beside each, `*_host_enqueue_us`: the host's wall time per launch for enqueuing them (wrapper and C entry, before any synchronise).

Shape: 4096 x 8 segments, r = 4 (config 2).  Obstacles: tools/moving_bench.py's line_tracks -- every trajectory has a set of its own of k
one-segment tracks at constant velocity that pass within 0.3 m of one of its interior waypoints, under way for 0.4 of the flight, so
they wait, move and arrive inside the flight.  One JSON line per measurement.  Needs the GPU: there is no CPU path."""
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
from moving_bench import line_tracks  # noqa: E402

CACHE_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--n-traj", type=int, default=4096)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    f64, i32 = torch.float64, torch.int32
    version = _lib.lib().uavqp_version
    version.restype = ctypes.c_char_p
    print(json.dumps(dict(library=version().decode())))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    with U.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        r, M, n = 4, 8, args.n_traj
        nc = 2 * r
        b = W.uniform_batch(2, n, M, r, time_mode="distance")
        wp = np.ascontiguousarray(b["waypoints"], dtype=np.float64).reshape(-1, 3)
        T0 = np.asarray(b["times"], dtype=np.float64).ravel()
        total, nco = n * M, 3 * nc * n * M
        d_T = up(T0)
        coeff0, status0 = torch.zeros(nco, dtype=f64, device=dev), torch.zeros(n, dtype=i32, device=dev)
        ctx.solve_batch_device(r, n, M, M, None, up(wp), d_T, up(np.asarray(b["bc"], dtype=np.float64)), coeff0, status0)
        ctx.synchronize()
        host_coeff = coeff0.cpu().numpy()
        host_obs = {k: line_tracks(wp, T0, n, M, r, k, 900 + k) for k in (1, 8)}
        obstacles = {k: dict({key: up(v) for key, v in h.items()}, n_obs=n * k, uniform_segments=1, n_sets=n) for k, h in host_obs.items()}

        one = 8 * (nco + total + 2 * total + 2 * n) + 4 * (4 * total + total + n + n)
        rot = max(4, min(64, -(-2 * CACHE_BYTES // one)))
        sets = [dict(coeff=coeff0.clone(), status=status0.clone(), T=d_T.clone(), gap=torch.zeros((total, 2), dtype=f64, device=dev),
                     where=torch.zeros((total, 4), dtype=i32, device=dev), peak=torch.zeros((n, 2), dtype=f64, device=dev),
                     sv=torch.zeros(total, dtype=i32, device=dev), v=torch.zeros(n, dtype=i32, device=dev)) for _ in range(rot)]

        def cert(k, depth):
            def fn(q):
                ctx.moving_certificate_device(r, n, M, None, q["T"], q["coeff"], obstacles[k], status=q["status"], gap_out=q["gap"],
                                              where_out=q["where"], peak_out=q["peak"], seg_verdict_out=q["sv"], verdict_out=q["v"], depth=depth)
            return fn

        # ---- the yardstick: groups of one vehicle + its 8 tracks for the separation certificate
        k = 8
        h = host_obs[k]
        na = n * (1 + k)
        so = np.zeros(na + 1, dtype=np.int64)
        so[1:] = np.cumsum(np.tile(np.array([M] + [1] * k), n))
        sT = np.concatenate([np.concatenate([T0[t * M:(t + 1) * M], h["times"][t * k:(t + 1) * k]]) for t in range(n)])
        oc = h["coeff"].reshape(n, k, 3 * nc)
        sc = np.concatenate([np.concatenate([host_coeff[3 * nc * M * t:3 * nc * M * (t + 1)], oc[t].ravel()]) for t in range(n)])
        start = np.concatenate([np.concatenate([[0.0], h["start"][t * k:(t + 1) * k]]) for t in range(n)])
        flight = float(T0.reshape(n, M).sum(axis=1).max())
        d_sso, d_sT, d_go, d_start = up(so.astype(np.int32)), up(sT), up(np.arange(0, na + 1, 1 + k, dtype=np.int32)), up(start)
        s_one = 8 * (sc.size + 2 * na) + 4 * (6 * na + n)
        s_rot = max(4, min(64, -(-2 * CACHE_BYTES // s_one)))
        ssets = [dict(coeff=up(sc), lower=torch.zeros(na, dtype=f64, device=dev), upper=torch.zeros(na, dtype=f64, device=dev),
                      where=torch.zeros((na, 4), dtype=i32, device=dev), v=torch.zeros(na, dtype=i32, device=dev),
                      gv=torch.zeros(n, dtype=i32, device=dev)) for _ in range(s_rot)]

        def sep(depth):
            def fn(q):
                ctx.separation_certificate_device(r, na, 0, d_sso, d_sT, q["coeff"], n_groups=n, group_offsets=d_go, start=d_start,
                                                  lower_out=q["lower"], upper_out=q["upper"], where_out=q["where"], verdict_out=q["v"],
                                                  group_verdict_out=q["gv"], depth=depth, n_cells=M, clock_start=0.0, dt=flight / M)
            return fn

        host_us = {}

        def timed(name, fn, pool):
            for j in range(2 * len(pool)):
                fn(pool[j % len(pool)])
            torch.cuda.synchronize()
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            for j in range(args.launches):
                fn(pool[j % len(pool)])
            host_us.setdefault(name, []).append(1e6 * (time.perf_counter() - t0) / args.launches)
            b_.record()
            torch.cuda.synchronize()
            return 1e3 * a.elapsed_time(b_) / args.launches

        fns = [(f"cert_k{k}_d{depth}", cert(k, depth), sets) for depth in (3, 5) for k in (1, 8)]
        fns += [(f"separation_workaround_k8_d{depth}", sep(depth), ssets) for depth in (3, 5)]
        us = {name: [timed(name, fn, pool) for _ in range(args.runs)] for name, fn, pool in fns}
        verdicts = {}
        for k in (1, 8):
            for depth in (3, 5):
                cert(k, depth)(sets[0])
                ctx.synchronize()
                v = sets[0]["v"].cpu().numpy()
                verdicts[f"k{k}_d{depth}"] = dict(certified=int((v & 1 != 0).sum()), violated=int((v & 2 != 0).sum()),
                                                  undecided=int((v == 0).sum()))
        print(json.dumps(dict(shape=f"config2_{n}x{M}_r{r}", n_traj=n, segments=total, launches=args.launches, runs=args.runs, buffer_sets=rot,
                              bytes_per_set=one, yardstick_buffer_sets=s_rot, yardstick_trajectories=na, verdicts_d_req_1=verdicts,
                              **{f"{k}_us": statistics.median(v) for k, v in us.items()}, **{f"{k}_us_min": min(v) for k, v in us.items()},
                              **{f"{k}_us_max": max(v) for k, v in us.items()},
                              **{f"{k}_host_enqueue_us": statistics.median(v) for k, v in host_us.items()})))


if __name__ == "__main__":
    main()
