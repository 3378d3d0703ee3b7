"""Timing of uavqp_solve_backward_device next to uavqp_solve_batch_device on the same buffers, for docs/measurement_log.md: 4096 x 8 and
65536 x 8 at r = 4, 65536 x 16 at r = 3 and BASELINE config 4's ragged batch (32768 trajectories, 4 .. 24 segments, r = 3).
Warm-up, HIP events around the repeats, buffer sets rotated through more memory than the caches hold (as bench.py does).
Algorithmic bytes of the backward pass: the forward's inputs + coeff and grad_coeff read, the three gradients written.
    python tools/adjoint_bench.py [--reps 100] [--only NAME]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import uav_motion_planning_amd as U  # noqa: E402
from uav_motion_planning_amd import workloads as W  # noqa: E402

SHAPES = {
    "4096x8_r4": lambda: (4, W.uniform_batch(2, 4096, 8, 4, time_mode="distance"), 8),
    "65536x8_r4": lambda: (4, W.uniform_batch(2, 65536, 8, 4, time_mode="distance"), 8),
    "65536x16_r3": lambda: (3, W.uniform_batch(1, 65536, 16, 3, time_mode="distance"), 16),
    "config4_ragged_r3": lambda: (3, W.ragged_batch(4, 32768, 3, m_lo=4, m_hi=24), 0),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--only", default=None)
    ap.add_argument("--rotate-mb", type=float, default=768.0, help="memory the rotating buffer sets cover (above the 256 MB of last-level cache)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    with U.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        for name, make in SHAPES.items():
            if a.only and a.only != name:
                continue
            r, b, uni = make()
            so_np = np.ascontiguousarray(b["seg_offsets"], dtype=np.int32)
            n, total, mmax = so_np.size - 1, int(so_np[-1]), int(np.max(np.diff(so_np)))
            so = None if uni else torch.from_numpy(so_np).to(dev)
            f64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)   # noqa: E731
            nco = 3 * 2 * r * total
            bytes_fwd = 8 * (3 * (total + n) + total + n * 6 * (r - 1)) + 8 * nco
            bytes_bwd = 8 * (3 * (total + n) + total + n * 6 * (r - 1)) + 2 * 8 * nco + 8 * (total + 3 * (total + n) + n * 6 * (r - 1)) + 4 * n
            n_sets = max(2, min(64, int(a.rotate_mb * 2 ** 20 / bytes_bwd) + 1))
            g0 = torch.randn(nco, dtype=torch.float64, device=dev)
            sets = [dict(wp=f64(b["waypoints"]).reshape(-1, 3), T=f64(b["times"]).ravel(), bc=f64(b["bc"]), coeff=torch.zeros(nco, dtype=torch.float64, device=dev),
                         st=torch.zeros(n, dtype=torch.int32, device=dev), g=g0.clone(), gT=torch.zeros(total, dtype=torch.float64, device=dev),
                         gW=torch.zeros((total + n, 3), dtype=torch.float64, device=dev), gB=torch.zeros((n, 2, r - 1, 3), dtype=torch.float64, device=dev))
                    for _ in range(n_sets)]

            def forward(s):
                ctx.solve_batch_device(r, n, uni, mmax, so, s["wp"], s["T"], s["bc"], s["coeff"], s["st"])

            def backward(s):
                ctx.solve_backward_device(r, n, uni, mmax, total, so, s["wp"], s["T"], s["bc"], s["coeff"], s["g"], grad_times=s["gT"],
                                          grad_waypoints=s["gW"], grad_bc=s["gB"], status=s["st"])

            def timed(fn, reps):
                for i in range(min(n_sets, 8)):
                    fn(sets[i % n_sets])
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(reps):
                    fn(sets[i % n_sets])
                e1.record()
                torch.cuda.synchronize(dev)
                return e0.elapsed_time(e1) * 1e3 / reps

            for s in sets:
                forward(s)
            fwd = [round(timed(forward, a.reps), 2) for _ in range(3)]
            bwd = [round(timed(backward, a.reps), 2) for _ in range(3)]
            assert bool((sets[0]["st"] == U.UAVQP_SOLVED).all()) and bool(torch.isfinite(sets[0]["gT"]).all())
            print(json.dumps(dict(shape=name, r=r, n_traj=n, total_segments=total, reps=a.reps, buffer_sets=n_sets,
                                  rotated_megabytes=round(n_sets * bytes_bwd / 2 ** 20, 1), forward_us=fwd, backward_us=bwd,
                                  backward_over_forward=round(min(bwd) / min(fwd), 2), forward_algorithmic_bytes=bytes_fwd, backward_algorithmic_bytes=bytes_bwd,
                                  forward_GBps=round(bytes_fwd / min(fwd) / 1e3, 1), backward_GBps=round(bytes_bwd / min(bwd) / 1e3, 1))), flush=True)
            del sets
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
