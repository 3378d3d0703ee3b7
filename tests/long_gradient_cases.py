"""Inputs and references shared by test_long_gradient_inputs.py (CPU) and test_gpu_long_gradients.py (-m gpu): the backward pass of the
equality solve, the closed-form time gradient and the duration optimiser from 25 to 96 segments.  numpy and the oracle only; no test
lives here.

Uniform batches of two trajectories in the shapes of test_solve_backward_contract.py's random_case (non-zero boundary derivatives, knot
spacing 0.5 / 2 / 4, T ~ U(0.7, 2), g ~ N(0, 1)) at the lengths where something changes: 25 the first count past the short tests, 32 / 33
the first workspace record past 32, 48 / 49 and 63 / 64 / 65 the forward's changes of kernel and host path, 96 the forward test's longest.
One ragged batch per r with short trajectories behind long ones in the same wave and T ~ U(0.2, 3).  No duration is below 0.2 s: below
that the double-precision reference (kkt_adjoint), not the kernel, becomes the limiting term at 64 snap segments.

References.  Waypoints / boundary derivatives: kkt_adjoint (dense double-precision KKT inverse), pinned by the CPU test against exact
differences of binary128 solves on a subset of the knots.  Durations: central differences of the binary128 minimiser at h = 1e-4 T_i and
h / 2 on the sampled durations {0, M // 2, M - 1, argmin T} -- of g . c* and, from the same solves, of the optimal cost J = c*' P c* --
kept in tests/golden/long_gradients.npz (tests/golden/gen_long_gradients.py writes it; the CPU test recomputes one case); in between,
kkt_adjoint's grad_times."""
import os

import numpy as np

from test_solve_backward_contract import kkt_adjoint, random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "long_gradients.npz")

UNIFORM = ((3, 33), (3, 49), (3, 64), (4, 25), (4, 32), (4, 48), (4, 63), (4, 65), (4, 96))
LANES = ((4, 49), (4, 64))      # the forward's lane layouts (uavqp_settings.generic_lanes_per_traj) are run at these two
RAGGED_LENGTHS = (1, 24, 25, 40, 63, 64, 96, 7)
RAGGED_MAX = 96
# The draw of the ragged batches.  With T ~ U(0.2, 3) the KKT matrix of a snap trajectory has a condition number of 1e12 .. 4e15 and
# kkt_adjoint, the double-precision reference, is off by 1e-14 .. 9e-12 of max|grad| from exact oracle differences depending on the
# draw (seven draws: worst per batch 8e-13 .. 8e-12).  This one leaves a factor 12 to the 1e-11 that test_long_gradient_inputs.py
# asks of the reference, so that the last bits of another LAPACK do not decide that test.
RAGGED_SEED = 4
T_MIN = 0.2
H_REL = 1e-4


def _pack(name, r, cases, uniform):
    lens = [c[2].size for c in cases]
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return dict(name=name, r=r, uniform=uniform, n=len(cases), so=so, lengths=np.array(lens), wp=np.vstack([c[0] for c in cases]),
                bc=np.array([c[1] for c in cases]), T=np.concatenate([c[2] for c in cases]), g=np.concatenate([c[3].ravel() for c in cases]))


def uniform_case(r, M, n=2):
    """n trajectories of M segments: random_case(r, M, seed) each."""
    return _pack(f"uniform_r{r}_M{M}", r, [random_case(r, M, 41000 + 1000 * r + 10 * M + j) for j in range(n)], True)


def ragged_case(r):
    """RAGGED_LENGTHS in that order, durations re-drawn from U(0.2, 3)."""
    cases = []
    for j, M in enumerate(RAGGED_LENGTHS):
        wp, bc, _, g = random_case(r, M, 43000 + 1000 * r + 100 * RAGGED_SEED + j)
        T = np.random.default_rng(47000 + 1000 * r + 100 * RAGGED_SEED + j).uniform(T_MIN, 3.0, size=M)
        cases.append((wp, bc, T, g))
    return _pack(f"ragged_r{r}", r, cases, False)


def all_cases():
    return [uniform_case(r, M) for r, M in UNIFORM + LANES] + [ragged_case(3), ragged_case(4)]


def case_by_name(name):
    if name.startswith("ragged"):
        return ragged_case(int(name[-1]))
    r, M = name.split("_")[1:]
    return uniform_case(int(r[1:]), int(M[1:]))


CASE_NAMES = [f"uniform_r{r}_M{M}" for r, M in UNIFORM] + ["ragged_r3", "ragged_r4"]
LANE_NAMES = [f"uniform_r{r}_M{M}" for r, M in LANES]


def traj(case, b):
    """(M, wp [M+1, 3], bc [2, r-1, 3], T [M], g [3, M, 2r]) of trajectory b."""
    s0, s1 = int(case["so"][b]), int(case["so"][b + 1])
    nc = 2 * case["r"]
    return s1 - s0, case["wp"][s0 + b:s1 + b + 1], case["bc"][b], case["T"][s0:s1], case["g"][3 * nc * s0:3 * nc * s1].reshape(3, s1 - s0, nc)


def sampled_durations(T):
    M = T.size
    return np.array(sorted({0, M // 2, M - 1, int(np.argmin(T))}))


def sampled_knots(M):
    return np.array(sorted({0, min(1, M), M // 2, max(M - 1, 0), M}))


def exact_linear_gradients_subset(oracle, r, T, g, knots):
    """exact_linear_gradients of the contract test on the knots `knots` and on all boundary derivatives: c* is linear in both, so one
    binary128 solve with a unit right-hand side (the same for the three axes) gives the exact column.  -> (gW [len(knots), 3], gB [2, r-1, 3])"""
    M = T.size
    gv = np.asarray(g).reshape(3, -1)
    zp, zb = np.zeros(M + 1), np.zeros(r - 1)
    gW, gB = np.zeros((len(knots), 3)), np.zeros((2, r - 1, 3))
    for j, k in enumerate(knots):
        gW[j] = gv @ oracle.solve_exact(r, np.eye(M + 1)[k], zb, zb, T)
    for d in range(r - 1):
        gB[0, d] = gv @ oracle.solve_exact(r, zp, np.eye(r - 1)[d], zb, T)
        gB[1, d] = gv @ oracle.solve_exact(r, zp, zb, np.eye(r - 1)[d], T)
    return gW, gB


def fd_sampled(oracle, r, wp, bc, T, g, idx, h_rel=H_REL):
    """Central differences in the durations `idx` at h_rel T_i and half of it, of phi = g . c* and of J = c*' P c* (binary128 minimiser,
    one set of solves for both).  -> (phi [len(idx), 2], J [len(idx), 2]); column 0 the step h, column 1 the step h / 2."""
    gv = np.asarray(g).reshape(3, -1)

    def both(Tq):
        c = [oracle.solve_exact(r, wp[:, ax], bc[0, :, ax], bc[1, :, ax], Tq) for ax in range(3)]
        return np.array([sum(float(gv[ax] @ c[ax]) for ax in range(3)), sum(2.0 * oracle.cost(r, Tq, c[ax]) for ax in range(3))])
    out = np.zeros((len(idx), 2, 2))
    for j, i in enumerate(idx):
        for k, h in enumerate((h_rel, h_rel / 2)):
            e = np.zeros(T.size)
            e[i] = h * T[i]
            out[j, k] = (both(T + e) - both(T - e)) / (2.0 * e[i])
    return out[:, :, 0], out[:, :, 1]


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def golden_fd(name, b):
    """(idx, phi [len(idx), 2], J [len(idx), 2]) of trajectory b of case `name` from the committed file."""
    z = golden()
    return z[f"{name}/{b}/idx"], z[f"{name}/{b}/phi"], z[f"{name}/{b}/J"]


_refs = {}


def references(oracle, case):
    """Per trajectory of the case, made once per session: dict(kkt=(gT, gW, gB) of kkt_adjoint, idx, phi, J from the golden file,
    rich = the Richardson estimate max|f_h - f_h/2| / max|grad_times| of phi's differences)."""
    if case["name"] not in _refs:
        out = []
        for b in range(case["n"]):
            M, wp, bc, T, g = traj(case, b)
            kkt = kkt_adjoint(oracle, case["r"], wp, bc, T, g)
            idx, phi, J = golden_fd(case["name"], b)
            assert np.array_equal(idx, sampled_durations(T)), "tests/golden/long_gradients.npz is not of these inputs: run gen_long_gradients.py"
            out.append(dict(kkt=kkt, idx=idx, phi=phi, J=J, rich=np.max(np.abs(phi[:, 0] - phi[:, 1])) / np.max(np.abs(kkt[0]))))
        _refs[case["name"]] = out
    return _refs[case["name"]]


_coeffs = {}


def oracle_coefficients(oracle, case):
    """The binary128 minimiser of the whole case rounded to double, flat in the C-ABI layout; made once per session."""
    if case["name"] not in _coeffs:
        ref, st = oracle.solve_exact_batch(case["r"], case["so"], case["wp"], case["T"], case["bc"])
        assert np.all(st == 0)
        _coeffs[case["name"]] = ref
    return _coeffs[case["name"]]
