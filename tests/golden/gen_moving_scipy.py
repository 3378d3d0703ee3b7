"""Generator of tests/golden/moving_scipy.json (CPU only; run from the repository root: python tests/golden/gen_moving_scipy.py).

Per trajectory of the batches of tests/moving_opt_reference.py: f at the start, the optimum of scipy's L-BFGS-B on the CPU reference
objective (tests/spacetime_reference.py lbfgsb on MovingProblem), f of the CPU transcription of the optimiser after the default number of
trials, and the moving-obstacle penalty and the smallest sampled gap at the start and at scipy's optimum.  Asserts that no trajectory
has to be left out of the comparison (f_start > 1.5 f_scipy, nothing outside the map) and prints the worst gap of the transcription: the
constant GAP_MOVING_AT_DEFAULT of tests/moving_opt_reference.py, also written into the file."""
import json
import os
import sys
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def one(job):
    from oracle import oracle
    import moving_opt_reference as MO
    import spacetime_reference as R
    r, kind, t = job
    oracle.build()
    prob = MO.problem_of(oracle, r, kind, t)
    start = prob.parts(prob.start_p, R.clamp_times(prob.start_T))
    sp = R.lbfgsb(prob)
    at = prob.parts(sp["p"], sp["T"])
    it = MO.iterate(prob)
    rec = dict(M=int(prob.M), f_start=float(start["f"]), f_scipy=float(sp["f"]), f_transcription=float(it["f"]),
               outside=int(max(start["outside"], sp["outside"], it["outside"])), phi_moving_start=float(start["phi_mov"]),
               phi_moving_scipy=float(at["phi_mov"]), phi_att_scipy=float(at["phi_att"]), min_gap_start=float(start["min_gap"]),
               min_gap_scipy=float(at["min_gap"]))
    rec["gap_transcription"] = (rec["f_transcription"] - rec["f_scipy"]) / (rec["f_start"] - rec["f_scipy"])
    return job, rec


def main():
    import moving_opt_reference as MO
    jobs = [(r, kind, t) for r, kind in MO.KINDS for t in range(MO.batch_of(r, kind)["seg_offsets"].size - 1)]
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        done = dict(pool.map(one, jobs, chunksize=1))
    out = {f"r{r}-{kind}": [done[j] for j in jobs if j[:2] == (r, kind)] for r, kind in MO.KINDS}
    worst = max(((rec["gap_transcription"], key, i) for key, recs in out.items() for i, rec in enumerate(recs)))
    ratio = min(rec["f_start"] / rec["f_scipy"] for recs in out.values() for rec in recs)
    for key, recs in out.items():
        for i, rec in enumerate(recs):
            assert rec["f_start"] > 1.5 * rec["f_scipy"] and rec["outside"] == 0, f"{key} trajectory {i} would be left out of the comparison"
            assert rec["phi_moving_start"] > 0, f"{key} trajectory {i}: no track comes inside D_o of the start trajectory"
    out["GAP_MOVING_AT_DEFAULT"] = dict(gap=float(f"{worst[0]:.3e}"), batch=worst[1], trajectory=worst[2], max_iters=MO.DEFAULT_MAX_ITERS)
    with open(os.path.join(HERE, "moving_scipy.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"{len(jobs)} trajectories; smallest f_start / f_scipy {ratio:.3f}; worst gap of the transcription after {MO.DEFAULT_MAX_ITERS} trials: "
          f"{worst[0]:.3e} at {worst[1]} trajectory {worst[2]}")
    for key, recs in out.items():
        if key == "GAP_MOVING_AT_DEFAULT":
            continue
        print(key, " ".join(f"{rec['gap_transcription']:.1e}" for rec in recs))
        print("   Phi_moving at the start:", " ".join(f"{rec['phi_moving_start']:.3g}" for rec in recs))
        print("   Phi_moving at scipy's optimum:", " ".join(f"{rec['phi_moving_scipy']:.3g}" for rec in recs))
        print("   smallest gap at the start / at scipy's optimum:", " ".join(f"{rec['min_gap_start']:.2f}/{rec['min_gap_scipy']:.2f}" for rec in recs))


if __name__ == "__main__":
    main()
