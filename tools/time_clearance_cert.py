"""The measurement of the certified clearance (docs/measurement_log.md).

    python tools/time_clearance_cert.py [--launches 50] [--reps 5] [--n-traj 4096] [--depths 4 6] [--once DEPTH]

Device time of one uavqp_clearance_certificate_device launch with every output, per depth: `--launches` launches between two events after
a warm-up, inputs and outputs rotating through enough sets of buffers to exceed the 256 MB last-level cache; median, min and max of
`--reps` such runs.  Beside it one uavqp_clearance_penalty_device launch (penalty, both gradients, min_dist, outside; 8 samples per
segment) on the same coefficients and map: the sampled test the certificate stands next to.  The counts of certified / violated /
undecided trajectories at each depth are printed with it.

Shape: 4096 x 8 segments, r = 4 (config 2), durations by distance; the map of tools/esdf_bench.py (200 x 200 x 50 voxels of 0.2 m, 60
pillars inflated by 0.2 m); d_req 0.5 m.  One JSON line per measurement.  `--once DEPTH` does one warm-up launch and one launch at that
depth and nothing else: the run to collect hardware counters on.  Needs the GPU: there is no CPU path."""
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
from uav_motion_planning_amd.esdf import EsdfMap  # noqa: E402

CACHE_BYTES = 256 << 20
D_REQ = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--n-traj", type=int, default=4096)
    ap.add_argument("--depths", type=int, nargs="+", default=[4, 6])
    ap.add_argument("--once", type=int, default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    f64, i32 = torch.float64, torch.int32
    version = _lib.lib().uavqp_version
    version.restype = ctypes.c_char_p
    print(json.dumps(dict(library=version().decode())))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    cloud = W.pillar_cloud(5, n_pillars=60, resolution=0.2)
    lo = cloud.min(axis=0) - 0.5
    with U.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        m = EsdfMap(ctx, (200, 200, 50), tuple(lo), 0.2)
        m.set_cloud(up(cloud), inflation=0.2)
        m.update()
        r, M, n = 4, 8, args.n_traj
        b = W.uniform_batch(2, n, M, r, time_mode="distance")
        total, nco = n * M, 3 * 2 * r * n * M
        d_wp, d_bc = up(np.asarray(b["waypoints"], dtype=np.float64).reshape(-1, 3)), up(np.asarray(b["bc"], dtype=np.float64))
        d_T = up(np.asarray(b["times"], dtype=np.float64).ravel())
        one = 8 * (nco + total + 2 * total + 2 * n) + 4 * (2 * total + 2 * n)
        rot = 2 if args.once is not None else max(2, min(256, -(-2 * CACHE_BYTES // one)))

        def new_set():
            return dict(T=d_T.clone(), coeff=torch.zeros(nco, dtype=f64, device=dev), status=torch.zeros(n, dtype=i32, device=dev),
                        clear=torch.zeros((total, 2), dtype=f64, device=dev), wit=torch.zeros(total, dtype=i32, device=dev),
                        peak=torch.zeros((n, 2), dtype=f64, device=dev), seg=torch.zeros(total, dtype=i32, device=dev),
                        word=torch.zeros(n, dtype=i32, device=dev), phi=torch.zeros(n, dtype=f64, device=dev),
                        g=torch.zeros(nco, dtype=f64, device=dev), gt=torch.zeros(total, dtype=f64, device=dev),
                        md=torch.zeros(n, dtype=f64, device=dev), out=torch.zeros(n, dtype=i32, device=dev))
        sets = [new_set() for _ in range(rot)]
        s = sets[0]
        ctx.solve_batch_device(r, n, M, M, None, d_wp, d_T, d_bc, s["coeff"], s["status"])
        ctx.synchronize()
        for q in sets[1:]:
            q["coeff"].copy_(s["coeff"])
            q["status"].copy_(s["status"])

        def certificate(depth):
            def fn(q):
                ctx.clearance_certificate_device(r, n, M, None, q["T"], q["coeff"], m, status=q["status"], clear_out=q["clear"],
                                                 witness_out=q["wit"], peak_out=q["peak"], seg_verdict_out=q["seg"], verdict_out=q["word"],
                                                 depth=depth, d_req=D_REQ)
            return fn

        def penalty(q):
            ctx.clearance_penalty_device(r, n, M, None, q["T"], q["coeff"], m, status=q["status"], penalty=q["phi"], grad_coeff=q["g"],
                                         grad_times=q["gt"], min_dist=q["md"], outside=q["out"], samples_per_seg=8, d_safe=D_REQ)

        if args.once is not None:
            certificate(args.once)(sets[0])
            certificate(args.once)(sets[1])
            ctx.synchronize()
            print(json.dumps(dict(measurement="clearance_certificate_once", depth=args.once, shape=f"config2_{n}x{M}_r{r}")))
            m.close()
            return

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

        ms = [timed(penalty) for _ in range(args.reps)]
        print(json.dumps(dict(measurement="clearance_penalty", shape=f"config2_{n}x{M}_r{r}", samples_per_seg=8, launches=args.launches,
                              buffer_sets=rot, ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))))
        for depth in args.depths:
            ms = [timed(certificate(depth)) for _ in range(args.reps)]
            word, clear = sets[0]["word"].cpu().numpy(), sets[0]["clear"].cpu().numpy()
            c, v = int(np.count_nonzero(word & _lib.UAVQP_CLEARANCE_CERTIFIED)), int(np.count_nonzero(word & _lib.UAVQP_CLEARANCE_VIOLATED))
            fin = np.isfinite(clear).all(axis=1)
            print(json.dumps(dict(measurement="clearance_certificate", shape=f"config2_{n}x{M}_r{r}", depth=depth, launches=args.launches,
                                  buffer_sets=rot, bytes_per_set=one, ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), d_req=D_REQ,
                                  map="200x200x50_at_0.2m", leaves_per_ms=total * (1 << depth) / statistics.median(ms),
                                  verdict=dict(certified=c, violated=v, undecided=n - c - v,
                                               outside=int(np.count_nonzero(word & _lib.UAVQP_CLEARANCE_OUTSIDE))),
                                  median_gap=float(np.median(clear[fin, 1] - clear[fin, 0])) if fin.any() else None)))
        m.close()


if __name__ == "__main__":
    main()
