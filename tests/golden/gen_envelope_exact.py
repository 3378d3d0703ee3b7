"""Generator of tests/golden/envelope_exact.json (CPU only, a few seconds; run from the repository root: python tests/golden/gen_envelope_exact.py).

Per recorded case of tests/envelope_reference.py (cases): the inputs (r, seg_offsets, times, coeff -- solved by the CPU oracle, or closed
forms) and the exact minimum and maximum over every whole segment of each quantity of uavqp_envelope_*, by mpmath at 60 digits
(exact_extrema), written as decimal strings of 40 digits."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import envelope_reference as E
    out = {}
    for name, c in E.cases().items():
        ex = E.exact_extrema(c["r"], c["seg_offsets"], c["times"], c["coeff"])
        out[name] = dict(r=c["r"], seg_offsets=[int(x) for x in c["seg_offsets"]], times=[float(x) for x in c["times"]],
                         coeff=[float(x) for x in c["coeff"]], range=ex["range"], norm=ex["norm"])
        print(name, len(c["times"]), "segments")
    with open(os.path.join(HERE, "envelope_exact.json"), "w") as fh:
        json.dump(dict(tilt_max=E.TILT_GOLDEN, cases=out), fh, indent=0)


if __name__ == "__main__":
    main()
