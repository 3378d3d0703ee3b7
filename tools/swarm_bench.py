"""Device time of one uavqp_swarm_penalty_device launch (docs/measurement_log.md), in the manner of
tools/spacetime_bench.py, beside one uavqp_flight_penalty_device launch on the same batch for scale.

    python tools/swarm_bench.py [--reps 9] [--warmup 20] [--launches 200] [--swarms 512] [--vehicles 8] [--segments 8] [--samples 64]

Batch: `--swarms` swarms of `--vehicles` vehicles of `--segments` segments, r = 4, laid by tests/swarm_reference.py: scene() through a
common region per swarm, so that the pair phase has work (the share of samples with a non-zero force is printed); the swarms on a grid
inside the 200 x 200 x 50 map of tools/waypoint_opt_bench.py, which the flight penalty samples.  Every output of both entries is asked for.
Each repetition: `--launches` launches of one entry between two events after a warm-up, the two entries alternating, outputs rotating
through four sets of buffers; per entry the median time per launch and the spread over the repetitions.  One JSON line per measurement.
Needs the GPU: there is no CPU path."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import uav_motion_planning_amd as U  # noqa: E402
from uav_motion_planning_amd import _lib  # noqa: E402
from uav_motion_planning_amd import workloads as W  # noqa: E402
from uav_motion_planning_amd.esdf import EsdfMap  # noqa: E402
import swarm_reference as S  # noqa: E402

ROT = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--swarms", type=int, default=512)
    ap.add_argument("--vehicles", type=int, default=8)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--samples", type=int, default=64)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/swarm_bench.py needs the GPU: there is no CPU path")
    dev = torch.device("cuda", 0)
    f64, i32 = torch.float64, torch.int32
    version = _lib.lib().uavqp_version
    version.restype = ctypes.c_char_p
    print(json.dumps(dict(library=version().decode())))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    r, G, A, M, N = 4, args.swarms, args.vehicles, args.segments, args.samples
    n, total = G * A, G * A * M
    rng = np.random.default_rng(1)
    side = int(np.ceil(np.sqrt(G)))
    wps, Ts, starts = [], [], []
    for g in range(G):
        # 36 x 36 m of the map's 40 x 40 m, 2 m from its faces
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
        d_wp, d_T, d_start = up(wp), up(T), up(start)
        d_bc = torch.zeros(n * 2 * (r - 1) * 3, dtype=f64, device=dev)
        d_go = up((np.arange(G + 1) * A).astype(np.int32))
        coeff, status = torch.zeros(3 * 2 * r * total, dtype=f64, device=dev), torch.zeros(n, dtype=i32, device=dev)
        ctx.solve_batch_device(r, n, M, M, None, d_wp, d_T, d_bc, coeff, status)
        ctx.synchronize()
        assert bool((status == U.UAVQP_SOLVED).all())

        def new_set():
            z = lambda k, t=f64: torch.zeros(k, dtype=t, device=dev)
            return dict(phi=z(G), g=z(3 * 2 * r * total), gt=z(total), gs=z(n), ms=z(n), phi_f=z(n), g_f=z(3 * 2 * r * total), gt_f=z(total),
                        peak=z(2 * n), md=z(n), out=z(n, i32))
        sets = [new_set() for _ in range(ROT)]

        def swarm(s):
            ctx.swarm_penalty_device(r, n, M, None, d_T, coeff, n_groups=G, group_offsets=d_go, start=d_start, status=status, penalty=s["phi"],
                                     grad_coeff=s["g"], grad_times=s["gt"], grad_start=s["gs"], min_sep=s["ms"], n_samples=N)

        def flight(s):
            ctx.flight_penalty_device(r, n, M, None, d_T, coeff, esdf, status=status, penalty=s["phi_f"], grad_coeff=s["g_f"], grad_times=s["gt_f"],
                                      peak=s["peak"], min_dist=s["md"], outside=s["out"])

        entries = {"swarm_penalty": swarm, "flight_penalty": flight}
        for fn in entries.values():
            for k in range(args.warmup):
                fn(sets[k % ROT])
        ctx.synchronize()
        s = sets[0]
        phi, ms, gt = s["phi"].cpu().numpy(), s["ms"].cpu().numpy(), s["gt"].cpu().numpy()
        shape = dict(swarms=G, vehicles=A, segments=M, r=r, n_samples=N, penalised_swarms=int(np.count_nonzero(phi > 0)),
                     vehicles_closer_than_d_safe=int(np.count_nonzero(ms < 1.0)), median_phi=float(np.median(phi)),
                     segments_with_gradient=int(np.count_nonzero(gt)))
        print(json.dumps(dict(shape=shape)))
        times = {name: [] for name in entries}
        for rep in range(args.reps):
            for name, fn in entries.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for k in range(args.launches):
                    fn(sets[k % ROT])
                e1.record()
                torch.cuda.synchronize()
                times[name].append(1e3 * e0.elapsed_time(e1) / args.launches)
        for name, t in times.items():
            print(json.dumps(dict(entry=name, us_per_launch_median=round(statistics.median(t), 2), us_min=round(min(t), 2), us_max=round(max(t), 2),
                                  reps=args.reps, launches=args.launches)))
        esdf.close()


if __name__ == "__main__":
    main()
