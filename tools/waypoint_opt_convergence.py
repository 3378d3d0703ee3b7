"""CPU: how many trials the waypoint optimiser needs (the default max_iters of uavqp_default_waypoint_opt_params).

Runs the numpy transcription of the iteration (tests/waypoint_opt_reference.py: the oracle's exact solve + the longdouble penalty) on the
scenes of tests/test_gpu_waypoint_opt.py and prints, per batch, how much of scipy L-BFGS-B's decrease (same start, same box as bounds) is
left after 8, 16, 32, 64 and 128 trials:  left = (f_k - f_scipy) / (f_start - f_scipy).  It also checks what the tests presuppose of their
cases: f_start > 1.5 f_scipy and no sample outside the map at the start, at scipy's optimum and at the transcription's result.
No GPU.    python tools/waypoint_opt_convergence.py [--seed-search]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import waypoint_opt_reference as R   # noqa: E402
from oracle import oracle            # noqa: E402

STEPS = (8, 16, 32, 64, 128)


def study(batch, label, quiet=False):
    """-> (worst left per step [5], all preconditions hold)"""
    r, n = batch["r"], batch["seg_offsets"].size - 1
    worst, ok = np.full(len(STEPS), -np.inf), True
    for t in range(n):
        wp, T, bc = R.split(batch, t)
        if T.size < 2:
            continue
        prob = R.Problem(oracle, r, wp, T, bc, smooth_weight=R.PARAMS["smooth_weight"])
        ref = R.lbfgsb(prob)
        run = R.iterate(prob, STEPS[-1])
        _, _, pen0, _ = prob.parts(prob.start)
        left = np.array([(run["history"][k - 1] - ref["f"]) / (run["f_start"] - ref["f"]) for k in STEPS])
        d0, d_safe = float(pen0["min_dist"][0]), prob.cp["d_safe"]
        fine = run["f_start"] > 1.5 * ref["f"] and int(pen0["outside"][0]) == 0 and ref["outside"] == 0 and run["outside"] == 0
        fine = fine and (d0 >= d_safe or run["min_dist"] > d0)    # a trajectory that starts too close ends farther away
        ok = ok and fine
        worst = np.maximum(worst, left)
        if not quiet:
            print(f"  {label} t={t:2d} M={T.size:2d}: f_start {run['f_start']:11.4e} f_scipy {ref['f']:11.4e} ratio {run['f_start'] / ref['f']:8.1f} "
                  f"left " + " ".join(f"{x:9.2e}" for x in left) + f"  min_dist {float(pen0['min_dist'][0]):6.3f} -> {run['min_dist']:6.3f} "
                  f"(scipy {ref['min_dist']:6.3f})" + ("" if fine else "   PRECONDITION FAILS"))
    return worst, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed-search", action="store_true", help="print the first seed from 1 whose ragged batch meets the preconditions, per r")
    args = ap.parse_args()
    oracle.build()
    if args.seed_search:
        for r in (3, 4):
            for seed in range(1, 50):
                if study(R.cases(r, seed=seed), "", quiet=True)[1]:
                    print(f"r = {r}: seed {seed}")
                    break
        return
    t0 = time.time()
    total = np.full(len(STEPS), -np.inf)
    print("left after".ljust(24) + " ".join(f"{k:9d}" for k in STEPS))
    for r in (3, 4):
        for label, batch in ((f"ragged r={r}", R.cases(r)), (f"uniform r={r}", R.uniform_cases(r))):
            worst, ok = study(batch, label)
            print(f"{label:24s}" + " ".join(f"{x:9.2e}" for x in worst) + ("" if ok else "   A PRECONDITION FAILS"))
            total = np.maximum(total, worst)
    print("worst of all".ljust(24) + " ".join(f"{x:9.2e}" for x in total))
    print(f"({time.time() - t0:.0f} s)")


if __name__ == "__main__":
    main()
