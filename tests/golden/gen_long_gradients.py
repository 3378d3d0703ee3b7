"""Generator of tests/golden/long_gradients.npz (CPU only, a few minutes; run from the repository root: python tests/golden/gen_long_gradients.py).

Per trajectory of every case of tests/long_gradient_cases.py: the sampled durations idx = {0, M // 2, M - 1, argmin T} and the central
differences of the CPU oracle's binary128 minimiser in them at h = 1e-4 T_i and h / 2 (fd_sampled): phi = g . c* and J = c*' P c*, each
[len(idx), 2].  Keys "<case>/<trajectory>/idx|phi|J".  tests/test_long_gradient_inputs.py recomputes one case and compares."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import long_gradient_cases as G
    from oracle import oracle
    oracle.build()
    out = {}
    for case in G.all_cases():
        t0 = time.perf_counter()
        for b in range(case["n"]):
            M, wp, bc, T, g = G.traj(case, b)
            idx = G.sampled_durations(T)
            phi, J = G.fd_sampled(oracle, case["r"], wp, bc, T, g, idx)
            out[f"{case['name']}/{b}/idx"], out[f"{case['name']}/{b}/phi"], out[f"{case['name']}/{b}/J"] = idx, phi, J
        print(f"{case['name']}: {time.perf_counter() - t0:.1f} s", flush=True)
    np.savez(os.path.join(HERE, "long_gradients.npz"), **out)


if __name__ == "__main__":
    main()
