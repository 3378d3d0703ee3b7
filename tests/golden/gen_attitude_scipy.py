"""Generator of tests/golden/attitude_scipy.json (CPU only; run from the repository root: python tests/golden/gen_attitude_scipy.py).

Per trajectory of the batches of tests/attitude_opt_reference.py: f at the start, the optimum of scipy's L-BFGS-B on the CPU reference
objective (tests/spacetime_reference.py lbfgsb on AttitudeProblem), f of the CPU transcription of the optimiser after the default number of
trials, and the attitude peaks at the start and at scipy's optimum.  Prints the worst gap of the transcription: the constant
GAP_ATTITUDE_AT_DEFAULT of tests/attitude_opt_reference.py."""
import json
import os
import sys
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402


def one(job):
    from oracle import oracle
    import attitude_opt_reference as AO
    import spacetime_reference as R
    r, kind, t = job
    oracle.build()
    prob = AO.problem_of(oracle, r, kind, t)
    start = prob.parts(prob.start_p, R.clamp_times(prob.start_T))
    sp = R.lbfgsb(prob)
    at = prob.parts(sp["p"], sp["T"])
    it = AO.iterate(prob)
    rec = dict(M=int(prob.M), f_start=float(start["f"]), f_scipy=float(sp["f"]), f_transcription=float(it["f"]),
               outside=int(max(start["outside"], sp["outside"], it["outside"])), phi_att_start=float(start["phi_att"]),
               phi_att_scipy=float(at["phi_att"]), attitude_peak_start=[float(x) for x in start["attitude_peak"]],
               attitude_peak_scipy=[float(x) for x in at["attitude_peak"]])
    rec["gap_transcription"] = (rec["f_transcription"] - rec["f_scipy"]) / (rec["f_start"] - rec["f_scipy"])
    return job, rec


def main():
    import attitude_opt_reference as AO
    jobs = [(r, kind, t) for r, kind in AO.KINDS for t in range(AO.batch_of(r, kind)["seg_offsets"].size - 1)]
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        done = dict(pool.map(one, jobs, chunksize=1))
    out = {f"r{r}-{kind}": [done[j] for j in jobs if j[:2] == (r, kind)] for r, kind in AO.KINDS}
    worst = max(((rec["gap_transcription"], key, i) for key, recs in out.items() for i, rec in enumerate(recs)))
    ratio = min(rec["f_start"] / rec["f_scipy"] for recs in out.values() for rec in recs)
    with open(os.path.join(HERE, "attitude_scipy.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"{len(jobs)} trajectories; smallest f_start / f_scipy {ratio:.3f}; worst gap of the transcription after {AO.DEFAULT_MAX_ITERS} trials: "
          f"{worst[0]:.3e} at {worst[1]} trajectory {worst[2]}")
    for key, recs in out.items():
        print(key, " ".join(f"{rec['gap_transcription']:.1e}" for rec in recs))
        print("   peaks at the start (f_hi f_lo tilt rate), max over the batch:", np.max([rec["attitude_peak_start"] for rec in recs], axis=0),
              "at scipy's optimum:", np.max([rec["attitude_peak_scipy"] for rec in recs], axis=0))


if __name__ == "__main__":
    main()
