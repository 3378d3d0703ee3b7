"""The measurement of the certified separation (docs/measurement_log.md), modelled on tools/time_clearance_cert.py.

    python tools/time_separation_cert.py [--launches 50] [--reps 5] [--swarms 512] [--vehicles 8] [--segments 8] [--cells 64]
                                         [--depths 0 2 4] [--once DEPTH]

Device time of one uavqp_separation_certificate_device launch with every output, per depth: `--launches` launches between two events
after a warm-up, inputs and outputs rotating through enough sets of buffers to exceed the 256 MB last-level cache; median, min and max
of `--reps` such runs.  Beside it one uavqp_swarm_penalty_device launch with every output on the same batch and clock (the sampled
term the certificate stands next to), timed in the same way in the same process, and one swarm of 128 vehicles of 2 segments at depth 2.
The counts of certified / violated / undecided vehicles at each depth are printed with the times.

Batch: the one of tools/swarm_bench.py -- `--swarms` swarms of `--vehicles` vehicles of `--segments` segments, r = 4, laid through a
common region per swarm by tests/swarm_reference.py: scene(); the window is `--cells` cells of 0.1 s; d_req 1.0 m.  One JSON line per
measurement.  `--once DEPTH` does one warm-up launch and one launch at that depth and nothing else: the run to collect hardware counters
on.  Needs the GPU: there is no CPU path."""
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
import swarm_reference as S  # noqa: E402

CACHE_BYTES = 256 << 20
D_REQ = 1.0


def lay(rng, G, A, M, N, radius=1.6):
    side = int(np.ceil(np.sqrt(G)))
    wps, Ts, starts = [], [], []
    for g in range(G):
        centre = (2.0 + 36.0 * ((g % side) + 0.5) / side, 2.0 + 36.0 * ((g // side) + 0.5) / side, 5.0)
        w, T, s = S.scene(rng, [M] * A, centre=centre, radius=radius, flight=0.1 * N * 0.8, start_span=(-0.05 * N * 0.1, 0.1 * N * 0.15))
        wps += w
        Ts += T
        starts.append(s)
    return np.concatenate(wps), np.concatenate(Ts), np.concatenate(starts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--swarms", type=int, default=512)
    ap.add_argument("--vehicles", type=int, default=8)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--depths", type=int, nargs="+", default=[0, 2, 4])
    ap.add_argument("--once", type=int, default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_separation_cert.py needs the GPU: there is no CPU path")
    dev = torch.device("cuda", 0)
    f64, i32 = torch.float64, torch.int32
    version = _lib.lib().uavqp_version
    version.restype = ctypes.c_char_p
    print(json.dumps(dict(library=version().decode())))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    r, N = 4, args.cells

    with U.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)

        def batch(G, A, M, radius, once):
            """-> (n, rotating buffer sets, bytes of one set) of G swarms of A vehicles of M segments, solved on the device"""
            n, total = G * A, G * A * M
            nco = 3 * 2 * r * total
            wp, T, start = lay(np.random.default_rng(1), G, A, M, N, radius)
            d_wp, d_bc = up(wp), torch.zeros(n * 2 * (r - 1) * 3, dtype=f64, device=dev)
            d_T, d_start, d_go = up(T), up(start), up((np.arange(G + 1) * A).astype(np.int32))
            one = 8 * (nco + total + n + 2 * n + nco + total + n + n + G) + 4 * (G + 1 + n + 4 * n + n + G)
            rot = 2 if once else max(2, min(256, -(-2 * CACHE_BYTES // one)))
            z = lambda k, t=f64: torch.zeros(k, dtype=t, device=dev)   # noqa: E731
            sets = [dict(T=d_T.clone(), start=d_start.clone(), go=d_go.clone(), coeff=z(nco), status=z(n, i32), lower=z(n), upper=z(n),
                         where=z(4 * n, i32), word=z(n, i32), gword=z(G, i32), phi=z(G), g=z(nco), gt=z(total), gs=z(n), ms=z(n))
                    for _ in range(rot)]
            s = sets[0]
            ctx.solve_batch_device(r, n, M, M, None, d_wp, d_T, d_bc, s["coeff"], s["status"])
            ctx.synchronize()
            assert bool((s["status"] == U.UAVQP_SOLVED).all())
            for q in sets[1:]:
                q["coeff"].copy_(s["coeff"])
                q["status"].copy_(s["status"])
            return dict(G=G, A=A, M=M, n=n, sets=sets, rot=rot, one=one)

        def certificate(B, depth):
            def fn(q):
                ctx.separation_certificate_device(r, B["n"], B["M"], None, q["T"], q["coeff"], n_groups=B["G"], group_offsets=q["go"],
                                                  start=q["start"], status=q["status"], lower_out=q["lower"], upper_out=q["upper"],
                                                  where_out=q["where"], verdict_out=q["word"], group_verdict_out=q["gword"], depth=depth,
                                                  n_cells=N, d_req=D_REQ)
            return fn

        def penalty(B):
            def fn(q):
                ctx.swarm_penalty_device(r, B["n"], B["M"], None, q["T"], q["coeff"], n_groups=B["G"], group_offsets=q["go"], start=q["start"],
                                         status=q["status"], penalty=q["phi"], grad_coeff=q["g"], grad_times=q["gt"], grad_start=q["gs"],
                                         min_sep=q["ms"], n_samples=N)
            return fn

        def timed(B, fn):
            for k in range(B["rot"]):
                fn(B["sets"][k % B["rot"]])
            torch.cuda.synchronize()
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(args.launches):
                fn(B["sets"][k % B["rot"]])
            b_.record()
            torch.cuda.synchronize()
            return 1e3 * a.elapsed_time(b_) / args.launches

        B = batch(args.swarms, args.vehicles, args.segments, 1.6, args.once is not None)
        shape = f"{B['G']}x{B['A']}x{B['M']}_r{r}_{N}cells"
        if args.once is not None:
            certificate(B, args.once)(B["sets"][0])
            certificate(B, args.once)(B["sets"][1])
            ctx.synchronize()
            print(json.dumps(dict(measurement="separation_certificate_once", depth=args.once, shape=shape)))
            return

        def report(B, shape, depth):
            us = [timed(B, certificate(B, depth)) for _ in range(args.reps)]
            q = B["sets"][0]
            word, lo, hi = q["word"].cpu().numpy(), q["lower"].cpu().numpy(), q["upper"].cpu().numpy()
            c, v = int(np.count_nonzero(word & _lib.UAVQP_SEPARATION_CERTIFIED)), int(np.count_nonzero(word & _lib.UAVQP_SEPARATION_VIOLATED))
            fin = np.isfinite(lo) & np.isfinite(hi)
            leaves = B["n"] * (N << depth)
            print(json.dumps(dict(measurement="separation_certificate", shape=shape, depth=depth, launches=args.launches, buffer_sets=B["rot"],
                                  bytes_per_set=B["one"], us=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2),
                                  d_req=D_REQ, entries_per_us=round(leaves / statistics.median(us), 1),
                                  verdict=dict(certified=c, violated=v, undecided=B["n"] - c - v,
                                               moving=int(np.count_nonzero(word & _lib.UAVQP_SEPARATION_MOVING))),
                                  median_gap=float(np.median(hi[fin] - lo[fin])) if fin.any() else None)))

        us = [timed(B, penalty(B)) for _ in range(args.reps)]
        print(json.dumps(dict(measurement="swarm_penalty", shape=shape, launches=args.launches, buffer_sets=B["rot"],
                              us=round(statistics.median(us), 2), us_min=round(min(us), 2), us_max=round(max(us), 2))))
        for depth in args.depths:
            report(B, shape, depth)
        B = batch(1, 128, 2, 8.0, False)
        report(B, f"1x128x2_r{r}_{N}cells", 2)


if __name__ == "__main__":
    main()
