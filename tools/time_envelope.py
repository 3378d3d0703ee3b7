"""The measurement of the certified bounds (docs/measurement_log.md).

    python tools/time_envelope.py [--launches 50] [--reps 5] [--n-traj 4096] [--depths 0 4 6]

Device time of one uavqp_envelope_device launch with every output and all limits set, per depth: `--launches` launches between two events
after a warm-up, inputs and outputs rotating through enough sets of buffers to exceed the 256 MB last-level cache; median, min and max
of `--reps` such runs.  Beside it one uavqp_limit_penalty_device launch (penalty, both gradients, peaks) on the same coefficients: the
sampled test the verdict replaces.  The counts of certified / violated / undecided trajectories at each depth are printed with it.

Shape: 4096 x 8 segments, r = 4 (config 2), durations by distance; limits at the median of the per-trajectory sampled peaks, so that
about half of the batch is on either side.  One JSON line per measurement.  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import uav_motion_planning_amd as U  # noqa: E402
from uav_motion_planning_amd import _lib  # noqa: E402
from uav_motion_planning_amd import workloads as W  # noqa: E402

CACHE_BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--n-traj", type=int, default=4096)
    ap.add_argument("--depths", type=int, nargs="+", default=[0, 4, 6])
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
        b = W.uniform_batch(2, n, M, r, time_mode="distance")
        total, nco = n * M, 3 * 2 * r * n * M
        d_wp, d_bc = up(np.asarray(b["waypoints"], dtype=np.float64).reshape(-1, 3)), up(np.asarray(b["bc"], dtype=np.float64))
        d_T = up(np.asarray(b["times"], dtype=np.float64).ravel())
        one = 8 * (nco + total + 48 * total + 20 * total + 20 * n) + 4 * (total + 2 * n)
        rot = max(2, min(64, -(-2 * CACHE_BYTES // one)))

        def new_set():
            return dict(T=d_T.clone(), coeff=torch.zeros(nco, dtype=f64, device=dev), status=torch.zeros(n, dtype=i32, device=dev),
                        range=torch.zeros((total, 4, 3, 4), dtype=f64, device=dev), norm=torch.zeros((total, 5, 4), dtype=f64, device=dev),
                        peak=torch.zeros((n, 5, 4), dtype=f64, device=dev), seg=torch.zeros(total, dtype=i32, device=dev),
                        word=torch.zeros(n, dtype=i32, device=dev), phi=torch.zeros(n, dtype=f64, device=dev),
                        g=torch.zeros(nco, dtype=f64, device=dev), gt=torch.zeros(total, dtype=f64, device=dev),
                        lpk=torch.zeros((n, 2), dtype=f64, device=dev))
        sets = [new_set() for _ in range(rot)]
        s = sets[0]
        ctx.solve_batch_device(r, n, M, M, None, d_wp, d_T, d_bc, s["coeff"], s["status"])
        ctx.limit_penalty_device(r, n, M, None, d_T, s["coeff"], status=s["status"], peak=s["lpk"], v_max=1.0, a_max=1.0)
        ctx.envelope_device(r, n, M, None, d_T, s["coeff"], status=s["status"], peak_out=s["peak"], depth=3)
        ctx.synchronize()
        for q in sets[1:]:
            q["coeff"].copy_(s["coeff"])
            q["status"].copy_(s["status"])
        lpk, epk = s["lpk"].cpu().numpy(), s["peak"].cpu().numpy()
        lim = dict(v_max=float(np.median(lpk[:, 0])), a_max=float(np.median(lpk[:, 1])), j_max=float(np.median(epk[:, 2, 2])),
                   f_min=float(np.median(epk[:, 3, 1])), f_max=float(np.median(epk[:, 3, 2])), tilt_max=0.6)

        def envelope(depth):
            def fn(q):
                ctx.envelope_device(r, n, M, None, q["T"], q["coeff"], status=q["status"], range_out=q["range"], norm_out=q["norm"],
                                    peak_out=q["peak"], seg_verdict_out=q["seg"], verdict_out=q["word"], depth=depth, **lim)
            return fn

        def limit(q):
            ctx.limit_penalty_device(r, n, M, None, q["T"], q["coeff"], status=q["status"], penalty=q["phi"], grad_coeff=q["g"], grad_times=q["gt"],
                                     peak=q["lpk"], v_max=lim["v_max"], a_max=lim["a_max"])

        def timed(fn):
            for k in range(rot):
                fn(sets[k % rot])
            torch.cuda.synchronize()
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(args.launches):
                fn(sets[k % rot])
            b_.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b_) / args.launches

        ms = [timed(limit) for _ in range(args.reps)]
        print(json.dumps(dict(measurement="limit_penalty", shape=f"config2_{n}x{M}_r{r}", launches=args.launches, buffer_sets=rot,
                              ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))))
        for depth in args.depths:
            ms = [timed(envelope(depth)) for _ in range(args.reps)]
            word = sets[0]["word"].cpu().numpy()
            counts = {}
            for k, name in enumerate(_lib.ENVELOPE_TESTS[:6]):
                c, v = int(np.count_nonzero((word >> (2 * k)) & 1)), int(np.count_nonzero((word >> (2 * k + 1)) & 1))
                counts[name] = dict(certified=c, violated=v, undecided=n - c - v)
            print(json.dumps(dict(measurement="envelope", shape=f"config2_{n}x{M}_r{r}", depth=depth, launches=args.launches, buffer_sets=rot,
                                  bytes_per_set=one, ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), limits=lim, verdict=counts)))


if __name__ == "__main__":
    main()
