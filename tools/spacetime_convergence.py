"""CPU: the test parameters and the default max_iters of the joint waypoint / duration optimiser (uavqp_default_spacetime_params;
DESIGN.md section 5.20).

Runs the numpy transcription of the iteration (tests/spacetime_reference.py: the oracle's exact solve + the two longdouble penalties) on the
scenes of tests/test_gpu_spacetime.py and prints, per batch, how much of scipy L-BFGS-B's decrease (same f, same start, same bounds) is left
after 32, 64, 128 and 256 trials:  left = (f_k - f_scipy) / (f_start - f_scipy).  The default max_iters is the smallest of the four whose
worst `left` is <= 5 % (256 if none).  It also checks what the tests presuppose of their cases (the rule in the docstring of
tests/spacetime_reference.py).
    python tools/spacetime_convergence.py               the table, GAP_AT_DEFAULT and the trajectory it is attained at
    python tools/spacetime_convergence.py --write-golden  the same, and f_start / f_scipy of every trajectory into tests/golden/spacetime_scipy.json
    python tools/spacetime_convergence.py --limits        sampled peaks at scipy's optimum with weight_v = weight_a = 0: the medians are LIMITS_OF[r]
    python tools/spacetime_convergence.py --seed-search   the first seed from 1 per r whose ragged and uniform batches meet the preconditions
    python tools/spacetime_convergence.py --method lbfgs  the same table for the limited-memory BFGS entry (tests/spacetime_lbfgs_reference.py) after
                                                          16, 32, 64 and 128 trials against the RECORDED scipy optima, GAP_LBFGS_AT_DEFAULT and its
                                                          trajectory, the settings memory 4 and max_backtracks 3, and the three feasibility
                                                          comparisons of the GPU test at 64 trials
No GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spacetime_reference as R   # noqa: E402
import spacetime_lbfgs_reference as Q   # noqa: E402
from oracle import oracle         # noqa: E402

NO_LIMITS = dict(weight_v=0.0, weight_a=0.0)


def problem(batch, t, **kw):
    wp, T, bc = R.split(batch, t)
    return R.Problem(oracle, batch["r"], wp, T, bc, **kw)


def study(batch, label, quiet=False, record=None):
    """-> (worst left per step, index of the trajectory with the worst left per step, all preconditions hold, trajectories over a limit
    at the optimum without the limit penalty)"""
    n = batch["seg_offsets"].size - 1
    worst, where, ok, over = np.full(len(R.STEPS), -np.inf), np.zeros(len(R.STEPS), dtype=int), True, 0
    for t in range(n):
        prob = problem(batch, t)
        rec = {}
        why = verdict(batch, t, rec)
        fine = why is None
        ref = rec.pop("_ref")
        run = rec.pop("_run", None)
        run = run or R.iterate(prob, R.STEPS[-1])          # (FEASIBILITY_ITERS = STEPS[-1]: its history holds every step)
        at_default = run
        over += int(max(rec.get("nolim_peak", [0.0])) > 1.0)
        left = np.array([(run["history"][k - 1] - ref["f"]) / (run["f_start"] - ref["f"]) for k in R.STEPS])
        ok = ok and fine
        if record is not None:
            record.append(rec)
        where = np.where(left > worst, t, where)
        worst = np.maximum(worst, left)
        if not quiet:
            print(f"  {label} t={t:2d} M={prob.M:2d}: f_start {run['f_start']:10.4e} f_scipy {ref['f']:10.4e} ratio {run['f_start'] / ref['f']:6.2f} left "
                  + " ".join(f"{x:9.2e}" for x in left) + f"  peaks {at_default['peak'][0]:5.2f} {at_default['peak'][1]:5.2f} min_dist {at_default['min_dist']:6.3f}"
                  f"  sum T {np.sum(prob.start_T):5.2f} -> {np.sum(at_default['T']):5.2f}" + ("" if fine else f"   RULE NOT MET: {why}"))
    return worst, where, ok, over


def verdict(batch, t, rec=None):
    """The seed rule on trajectory t: None, or the first reason why it is not met.  Cheapest checks first.  rec (a dict) receives what
    tests/golden/spacetime_scipy.json records of the trajectory."""
    prob = problem(batch, t)
    d_safe = prob.cp["d_safe"]
    start = prob.parts(prob.start_p, R.clamp_times(prob.start_T))
    ref = R.lbfgsb(prob)
    if rec is not None:
        rec.update(M=int(prob.M), f_start=float(start["f"]), f_scipy=float(ref["f"]), outside=int(ref["outside"]), _ref=ref)
    if not start["f"] > 1.5 * ref["f"]:
        return f"f_start = {start['f'] / ref['f']:.2f} f_scipy"
    if start["outside"] or ref["outside"]:
        return "a sample outside the map at the start or at scipy's optimum"
    run = R.iterate(prob, R.FEASIBILITY_ITERS)
    if rec is not None:
        rec.update(_run=run)
    if run["outside"]:
        return "a sample outside the map at the transcription's result"
    # smaller peaks than the optimum without the limit penalty, wherever that optimum exceeds a limit
    nolim = R.lbfgsb(problem(batch, t, limits=NO_LIMITS))
    if rec is not None:
        rec.update(nolim_peak=[float(x) for x in nolim["peak"]])
    for k in range(2):
        if nolim["peak"][k] > 1.0 and not run["peak"][k] < nolim["peak"][k]:
            return f"peak {k}: {run['peak'][k]:.4f} at the result, {nolim['peak'][k]:.4f} at the optimum without the limit penalty"
    # a larger smallest distance than the optimum without the clearance penalty, wherever that optimum comes closer than d_safe
    # (a trajectory of one segment has no waypoint to move)
    noclr = R.lbfgsb(problem(batch, t, clearance=dict(weight=0.0)))
    if rec is not None:
        rec.update(noclr_min_dist=float(noclr["min_dist"]))
    if prob.M > 1 and noclr["min_dist"] < d_safe and not run["min_dist"] > noclr["min_dist"]:
        return f"min_dist {run['min_dist']:.4f} at the result, {noclr['min_dist']:.4f} at the optimum without the clearance penalty"
    # ... and the same against the transcription's OWN runs with the weights zeroed: what tests/test_gpu_spacetime.py asserts of the device
    nolim_run = R.iterate(problem(batch, t, limits=NO_LIMITS), R.FEASIBILITY_ITERS)
    noclr_run = R.iterate(problem(batch, t, clearance=dict(weight=0.0)), R.FEASIBILITY_ITERS)
    if nolim_run["outside"] or noclr_run["outside"]:
        return "a sample outside the map in a run with a weight zeroed"
    for k in range(2):
        if nolim_run["peak"][k] > 1.0 and not run["peak"][k] < nolim_run["peak"][k]:
            return f"peak {k}: {run['peak'][k]:.4f} at the result, {nolim_run['peak'][k]:.4f} in the run without the limit penalty"
    if prob.M > 1 and noclr_run["min_dist"] < d_safe and not run["min_dist"] > noclr_run["min_dist"]:
        return f"min_dist {run['min_dist']:.4f} at the result, {noclr_run['min_dist']:.4f} in the run without the clearance penalty"
    return None


def check_seed(r, seed):
    """None if the ragged batch (seed) and the uniform batch (100 + seed) meet the whole rule, else the first reason why not."""
    oracle.build()
    for kind, batch in (("ragged", R.cases(r, seed=seed)), ("uniform", R.uniform_cases(r, seed=seed))):
        Ms = np.diff(batch["seg_offsets"])
        over, close, recs = 0, 0, []
        for t in np.argsort(Ms, kind="stable"):                  # (short trajectories first: they are cheap and fail most often)
            rec = {}
            why = verdict(batch, int(t), rec)
            if why:
                return f"{kind} trajectory {t}: {why}"
            over += int(max(rec["nolim_peak"]) > 1.0)
            close += int(Ms[t] > 1 and rec["noclr_min_dist"] < R.CLEARANCE["d_safe"])
        if 2 * over < Ms.size or 2 * close < Ms.size:
            return f"{kind}: {over} of {Ms.size} over a limit, {close} closer than d_safe at the optima without the penalties: fewer than half"
    return None


def batches(r):
    return (("ragged", R.cases(r)), ("uniform", R.uniform_cases(r)))


def lbfgs_table(rs):
    """The study of the limited-memory BFGS entry: gaps against the recorded scipy optima, and the feasibility comparisons at 64 trials."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "spacetime_scipy.json")))
    settings = (("memory 8, max_backtracks 6", {}), ("memory 4", dict(memory=4)), ("max_backtracks 3", dict(max_backtracks=3)))
    d_safe = R.CLEARANCE["d_safe"]
    for name, kw in settings:
        print(f"{name}: left after".ljust(44) + " ".join(f"{k:9d}" for k in Q.STEPS) + f"   gradient descent after {R.DEFAULT_MAX_ITERS}")
        total, at = np.full(len(Q.STEPS), -np.inf), [None] * len(Q.STEPS)
        for r in rs:
            for kind, batch in batches(r):
                n = batch["seg_offsets"].size - 1
                worst, where, gd, met, n_over, n_close = np.full(len(Q.STEPS), -np.inf), np.zeros(len(Q.STEPS), dtype=int), -np.inf, 0, 0, 0
                for t in range(n):
                    rec = golden[f"r{r}-{kind}"][t]
                    run = Q.iterate_lbfgs(problem(batch, t), Q.STEPS[-1], **kw)
                    assert abs(run["f_start"] - rec["f_start"]) <= 1e-9 * rec["f_start"], "the recorded results belong to other cases"
                    left = np.array([(run["history"][k - 1] - rec["f_scipy"]) / (run["f_start"] - rec["f_scipy"]) for k in Q.STEPS])
                    where = np.where(left > worst, t, where)
                    worst = np.maximum(worst, left)
                    if kw:
                        continue
                    old = R.iterate(problem(batch, t), R.DEFAULT_MAX_ITERS)
                    gd = max(gd, (old["f"] - rec["f_scipy"]) / (old["f_start"] - rec["f_scipy"]))
                    # the three comparisons of the GPU test, all runs at FEASIBILITY_ITERS trials
                    res = Q.iterate_lbfgs(problem(batch, t), Q.FEASIBILITY_ITERS)
                    nolim = Q.iterate_lbfgs(problem(batch, t, limits=NO_LIMITS), Q.FEASIBILITY_ITERS)
                    noclr = Q.iterate_lbfgs(problem(batch, t, clearance=dict(weight=0.0)), Q.FEASIBILITY_ITERS)
                    over = nolim["peak"] > 1.0
                    close = problem(batch, t).M > 1 and noclr["min_dist"] < d_safe
                    fine = (np.all(res["peak"][over] < nolim["peak"][over]) and (not close or res["min_dist"] > noclr["min_dist"])
                            and res["outside"] == 0 and nolim["outside"] == 0 and noclr["outside"] == 0)
                    met, n_over, n_close = met + int(fine), n_over + int(over.any()), n_close + int(close)
                    if not fine:
                        print(f"  {kind} r={r} t={t}: A FEASIBILITY COMPARISON FAILS at {Q.FEASIBILITY_ITERS} trials: peaks {res['peak']} against "
                              f"{nolim['peak']}, min_dist {res['min_dist']:.4f} against {noclr['min_dist']:.4f}")
                print(f"{kind + f' r={r}':44s}" + " ".join(f"{x:9.2e}" for x in worst) + (f"   {gd:9.2e}" if not kw else "")
                      + ("" if kw else f"   feasibility at {Q.FEASIBILITY_ITERS} trials: {met} of {n} meet all comparisons, {n_over} over a limit, "
                                       f"{n_close} closer than d_safe without the penalties"))
                for k in range(len(Q.STEPS)):
                    if worst[k] > total[k]:
                        total[k], at[k] = worst[k], (r, kind, int(where[k]))
        print("worst of all".ljust(44) + " ".join(f"{x:9.2e}" for x in total))
        if not kw:
            k = Q.STEPS.index(Q.DEFAULT_MAX_ITERS)
            print(f"default max_iters = {Q.DEFAULT_MAX_ITERS}: GAP_LBFGS_AT_DEFAULT = {total[k]:.3e} at GAP_LBFGS_CASE = {at[k]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", choices=("gd", "lbfgs"), default="gd", help="lbfgs: the table of the limited-memory BFGS entry")
    ap.add_argument("--limits", action="store_true")
    ap.add_argument("--seed-search", action="store_true")
    ap.add_argument("--write-golden", action="store_true")
    ap.add_argument("--jobs", type=int, default=8, help="seeds tried side by side by --seed-search")
    ap.add_argument("--r", type=int, nargs="+", default=[3, 4])
    args = ap.parse_args()
    oracle.build()
    t0 = time.time()
    if args.method == "lbfgs":
        lbfgs_table(args.r)
        print(f"({time.time() - t0:.0f} s)")
        return
    if args.limits:
        for r in (3, 4):
            v, a = [], []
            for kind, batch in batches(r):
                for t in range(batch["seg_offsets"].size - 1):
                    q = R.lbfgsb(problem(batch, t, limits=NO_LIMITS))
                    v.append(q["peak"][0] * R.LIMITS_OF[r]["v_max"])
                    a.append(q["peak"][1] * R.LIMITS_OF[r]["a_max"])
            print(f"r = {r}, {len(v)} trajectories: sampled peak speed min / median / max {min(v):.3f} / {np.median(v):.3f} / {max(v):.3f} m/s, "
                  f"acceleration {min(a):.3f} / {np.median(a):.3f} / {max(a):.3f} m/s^2")
            print(f"LIMITS_OF[{r}]: v_max = {np.floor(10 * np.median(v)) / 10:.1f}, a_max = {np.floor(10 * np.median(a)) / 10:.1f}")
        return
    if args.seed_search:
        # (seeds are tried side by side, args.jobs at a time; the answer is the FIRST seed from 1 that passes, whatever finishes first)
        from multiprocessing import Pool
        for r in args.r:
            seed, found = 1, None
            with Pool(args.jobs) as pool:
                while found is None and seed < 200:
                    chunk = list(range(seed, seed + args.jobs))
                    for s_, why in zip(chunk, pool.starmap(check_seed, [(r, s_) for s_ in chunk])):
                        print(f"r = {r}: seed {s_} {why or 'meets the rule'}", flush=True)
                        if why is None and found is None:
                            found = s_
                    seed += args.jobs
            print(f"r = {r}: SEEDS[{r}] = {found}", flush=True)
        return
    total, at, golden = np.full(len(R.STEPS), -np.inf), [None] * len(R.STEPS), {}
    print("left after".ljust(24) + " ".join(f"{k:9d}" for k in R.STEPS))
    for r in args.r:
        for kind, batch in batches(r):
            golden[f"r{r}-{kind}"] = []
            worst, where, ok, over = study(batch, f"{kind} r={r}", record=golden[f"r{r}-{kind}"])
            n = batch["seg_offsets"].size - 1
            print(f"{kind + f' r={r}':24s}" + " ".join(f"{x:9.2e}" for x in worst) + f"   {over} of {n} over a limit without the limit penalty"
                  + ("" if ok and 2 * over >= n else "   A PRECONDITION FAILS"))
            for k in range(len(R.STEPS)):
                if worst[k] > total[k]:
                    total[k], at[k] = worst[k], (r, kind, int(where[k]))
    print("worst of all".ljust(24) + " ".join(f"{x:9.2e}" for x in total))
    pick = next((k for k in range(len(R.STEPS)) if total[k] <= 0.05), len(R.STEPS) - 1)
    print(f"default max_iters = {R.STEPS[pick]}: GAP_AT_DEFAULT = {total[pick]:.3e} at GAP_CASE = {at[pick]}")
    if args.write_golden:
        if tuple(args.r) != (3, 4):   # (a partial study keeps the other orders' records)
            golden = dict(json.load(open(os.path.join(ROOT, "tests", "golden", "spacetime_scipy.json"))), **golden)
        with open(os.path.join(ROOT, "tests", "golden", "spacetime_scipy.json"), "w") as fh:
            json.dump(golden, fh, indent=1)
    print(f"({time.time() - t0:.0f} s)")


if __name__ == "__main__":
    main()
