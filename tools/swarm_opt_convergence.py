#!/usr/bin/env python3
"""CPU study of the swarm optimiser (tests/swarm_opt_reference.py: the transcription of include/uavqp.h against scipy's L-BFGS-B on all
variables of a swarm).  No GPU.

  swarm_opt_convergence.py                  the gap table: per swarm of the four test batches the fraction of scipy's decrease the
                                            transcription leaves after 16 / 32 / 64 / 128 trials, and the worst per column
  swarm_opt_convergence.py --write-golden   the same, and tests/golden/swarm_opt_scipy.json (results only)
  swarm_opt_convergence.py --seed-search    the first seed per r for which the conditions of tests/test_swarm_opt_contract.py hold

Per swarm it also runs the transcription with swarm weight = 0 (what the vehicles do when they do not see one another) and records the
smallest separations of both runs."""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "swarm_opt_scipy.json")


def one(job):
    r, kind, g, seed, with_scipy = job
    from oracle import oracle
    import swarm_opt_reference as O
    oracle.build()
    b = O.batch_of(r, kind, seed)
    prob = O.SwarmProblem.of_batch(oracle, b, g)
    run = O.iterate_swarm(prob, O.STEPS[-1])
    off = O.iterate_swarm(O.SwarmProblem.of_batch(oracle, b, g, swarm=dict(weight=0.0)), O.STEPS[-1])
    rec = dict(r=r, kind=kind, g=g, Ms=[int(v.M) for v in prob.veh], f_start=run["f_start"], phi_swarm_start=float(prob.parts(*prob.start())["phi_swarm"]),
               f_after={str(n): float(run["history"][n - 1]) for n in O.STEPS}, accepted=run["accepted"],
               outside=int(sum(q["outside"] for q in run["parts"]) + sum(q["outside"] for q in off["parts"])),
               min_sep=float(np.min(run["min_sep"])), noswarm_min_sep=float(np.min(off["min_sep"])))
    if with_scipy:
        ref = O.lbfgsb_swarm(prob)
        rec["f_scipy"] = ref["f"]
        rec["scipy_min_sep"] = float(np.min(ref["min_sep"]))
        rec["gap"] = {str(n): (rec["f_after"][str(n)] - ref["f"]) / (run["f_start"] - ref["f"]) for n in O.STEPS}
    return rec


def jobs(seed_of, with_scipy):
    import swarm_opt_reference as O
    return [(r, kind, g, seed_of[r], with_scipy) for r in (3, 4) for kind, groups in (("ragged", O.RAGGED), ("uniform", O.UNIFORM))
            for g in range(len(groups))]


def holds(recs, d_safe):
    """the conditions of the contract test on the records of one r"""
    multi = [q for q in recs if len(q["Ms"]) > 1]
    apart = [q for q in multi if q["noswarm_min_sep"] < d_safe and q["min_sep"] > q["noswarm_min_sep"]]
    return all(q["outside"] == 0 for q in recs) and all(q["phi_swarm_start"] > 0.0 for q in multi) and 2 * len(apart) >= len(recs)


def main():
    import swarm_opt_reference as O
    ap = argparse.ArgumentParser()
    ap.add_argument("--write-golden", action="store_true")
    ap.add_argument("--seed-search", action="store_true")
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    with multiprocessing.Pool(a.procs) as pool:
        if a.seed_search:
            for r in (3, 4):
                for seed in range(1, 33):
                    recs = [q for q in pool.map(one, jobs({3: seed, 4: seed}, False)) if q["r"] == r]
                    ok = holds(recs, O.SWARM["d_safe"])
                    print(f"r={r} seed={seed}: {'holds' if ok else 'fails'}  " + " ".join(
                        f"[{len(q['Ms'])}: {q['noswarm_min_sep']:.2f}->{q['min_sep']:.2f} out {q['outside']}]" for q in recs), flush=True)
                    if ok:
                        break
            return
        recs = pool.map(one, jobs(O.SEEDS, True))
    print("  r kind     g  A   f_start      f_scipy      " + "  ".join(f"gap@{n:<5d}" for n in O.STEPS) + "  min_sep (weight 0 -> penalised, scipy)")
    for q in recs:
        print(f"  {q['r']} {q['kind']:8s} {q['g']}  {len(q['Ms'])}  {q['f_start']:.5e}  {q['f_scipy']:.5e}  "
              + "  ".join(f"{q['gap'][str(n)]:.3e}" for n in O.STEPS) + f"  {q['noswarm_min_sep']:.3f} -> {q['min_sep']:.3f}, {q['scipy_min_sep']:.3f}")
    for n in O.STEPS:
        worst = max(recs, key=lambda q: q["gap"][str(n)])
        print(f"worst gap after {n:3d} trials: {worst['gap'][str(n)]:.3e}  (r={worst['r']} {worst['kind']} swarm {worst['g']})")
    for r in (3, 4):
        print(f"r={r}: the contract's conditions {'hold' if holds([q for q in recs if q['r'] == r], O.SWARM['d_safe']) else 'FAIL'}")
    if a.write_golden:
        out = {}
        for q in recs:
            out.setdefault(f"r{q['r']}-{q['kind']}", []).append({k: v for k, v in q.items() if k not in ("r", "kind", "g")})
        with open(GOLDEN, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", GOLDEN)


if __name__ == "__main__":
    main()
