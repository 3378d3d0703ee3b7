"""The references of test_gpu_long_gradients.py, checked on the CPU oracle alone (no GPU): every bound that the GPU test relies on is
met by the references themselves, with room to spare.

  * kkt_adjoint (dense double-precision KKT inverse, the reference for grad_waypoints / grad_bc on every element) against exact
    differences of binary128 solves on the knots {0, 1, M // 2, M - 1, M} and all boundary derivatives: 1e-11 of max|grad|, a hundredth
    of the 1e-9 the device is held to (measured over these cases: see docs/measurement_log.md, "Gradients on long trajectories").
  * the central differences of the binary128 minimiser in tests/golden/long_gradients.npz: Richardson estimate (h against h / 2) below
    1e-5, the project's rule, for g . c* and for the optimal cost; kkt_adjoint's grad_times, the reference for the durations in between,
    within 2 x that estimate of them on the sampled durations.
  * the file is what its generator writes: one case is recomputed from scratch."""
import numpy as np
import pytest

import long_gradient_cases as G

LINEAR_TOL = 1e-11


@pytest.mark.parametrize("name", G.CASE_NAMES + G.LANE_NAMES)
def test_references_meet_their_bounds(oracle, name):
    case = G.case_by_name(name)
    r = case["r"]
    assert np.min(case["T"]) >= G.T_MIN
    refs = G.references(oracle, case)
    for b in range(case["n"]):
        M, wp, bc, T, g = G.traj(case, b)
        gT, gW, gB = refs[b]["kkt"]
        knots = G.sampled_knots(M)
        xW, xB = G.exact_linear_gradients_subset(oracle, r, T, g, knots)
        ew = np.max(np.abs(gW[knots] - xW)) / np.max(np.abs(gW))
        eb = np.max(np.abs(gB - xB)) / np.max(np.abs(gB))
        idx, phi, J, rich = refs[b]["idx"], refs[b]["phi"], refs[b]["J"], refs[b]["rich"]
        et = np.max(np.abs(gT[idx] - phi[:, 1])) / np.max(np.abs(gT))
        rich_J = np.max(np.abs(J[:, 0] - J[:, 1])) / np.max(np.abs(J[:, 1]))
        print(f"{name} trajectory {b} (M={M}, min T {T.min():.3f}): kkt_adjoint vs exact differences waypoints {ew:.3e}, bc {eb:.3e}; "
              f"Richardson g.c* {rich:.3e}, cost {rich_J:.3e}; |kkt grad_times - fd| / max|grad| {et:.3e} = {et / rich:.2f} x Richardson")
        assert ew <= LINEAR_TOL and eb <= LINEAR_TOL, (b, ew, eb)
        assert rich < 1e-5 and rich_J < 1e-5, (b, rich, rich_J)
        assert et <= 2.0 * rich, (b, et, rich)


def test_the_shapes_are_those_the_gpu_test_needs():
    ragged = G.ragged_case(4)
    assert tuple(ragged["lengths"]) == (1, 24, 25, 40, 63, 64, 96, 7) and int(ragged["lengths"].max()) == G.RAGGED_MAX
    assert [(c["r"], int(c["lengths"][0])) for c in G.all_cases()[:len(G.UNIFORM)]] == list(G.UNIFORM)
    for case in G.all_cases():
        assert case["wp"].shape == (int(case["so"][-1]) + case["n"], 3) and case["g"].size == 6 * case["r"] * int(case["so"][-1])
        assert np.all(case["bc"] != 0.0)
        for b in range(case["n"]):
            M, _, _, T, _ = G.traj(case, b)
            idx = G.sampled_durations(T)
            assert 0 in idx and M - 1 in idx and M // 2 in idx and int(np.argmin(T)) in idx


def test_the_golden_file_is_what_the_generator_writes(oracle):
    case = G.uniform_case(3, 33)
    for b in range(case["n"]):
        M, wp, bc, T, g = G.traj(case, b)
        idx, phi, J = G.golden_fd(case["name"], b)
        assert np.array_equal(idx, G.sampled_durations(T))
        phi2, J2 = G.fd_sampled(oracle, case["r"], wp, bc, T, g, idx)
        # (differences of doubles divided by 1e-4 T: the last bits of another libquadmath may show at 1e-12)
        assert np.max(np.abs(phi2 - phi)) <= 1e-9 * np.max(np.abs(phi)) and np.max(np.abs(J2 - J)) <= 1e-9 * np.max(np.abs(J))
