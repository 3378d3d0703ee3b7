"""The inputs of test_gpu_long_trajectories.py, checked on the references alone (no GPU): the OSQP port solves every problem of the
cases it is the second reference for, its solutions pass the optimality certificate at the thresholds the GPU test uses, the 63-segment
batches have active constraints in the upper halves of the 64-bit working-set words (so that the GPU test can demand such bits), and
the certificate notices a coefficient of a late segment that is off by 1e-6 relative."""
import numpy as np
import pytest

import long_trajectory_cases as L

PRIM, STAT, COMP = 1e-9, 1e-7, 1e-6        # test_gpu_rows.py / test_gpu_corridor.py


def _n(r):
    return 24 if r == 3 else 12


@pytest.mark.parametrize("r,M,K", [(3, 63, 2), (4, 63, 1), (3, 33, 1)])
def test_port_solutions_pass_the_certificate_and_use_the_upper_bits(oracle, r, M, K):
    from oracle.certificates import kkt_certificate_rows
    n = _n(r)
    case = L.uniform_case(r, M, K, n)
    ref, solved, st = L.port_solve(oracle, case)
    assert solved.all(), st
    x = ref.reshape(n, 3, 2 * r * M)
    worst = np.zeros(3)
    high_box = high_row = vel_rows = 0
    hi_mask = ~((1 << 32) - 1)
    for k in range(n):
        M_, T, wp, bc, lo, hi, rows = L.trajectory_of(case, k)
        for ax in range(3):
            args = (T, x[k, ax], wp[:, ax], bc[0, :, ax], bc[1, :, ax], lo[1:M, ax], hi[1:M, ax], L.certificate_rows(rows, ax))
            worst = np.maximum(worst, kkt_certificate_rows(r, M, *args))
            bits = L.active_bits_from_solution(oracle, r, M, K, *args)
            high_box += bin((bits["box_lo"] | bits["box_hi"]) & hi_mask).count("1")
            high_row += bin((bits["row_lo"][0] | bits["row_hi"][0]) & hi_mask).count("1")
            if K == 2:
                vel_rows += bin(bits["row_lo"][1] | bits["row_hi"][1]).count("1")
    print(f"({r}, {M}, {K}) port certificate {worst}, active boxes >= 32: {high_box}, position rows >= 32: {high_row}, velocity rows: {vel_rows}")
    assert worst[0] < PRIM and worst[1] < STAT and worst[2] < COMP, worst
    if M == 63:
        assert high_box >= 1 and high_row >= 1
    if (r, M, K) == (3, 63, 2):
        assert vel_rows >= 1
    # one coefficient of a segment >= 32 off by 1e-6 relative: no longer a minimiser
    k, ax, seg = n // 2, 1, M - 5 if M == 63 else 32
    assert seg >= 32
    M_, T, wp, bc, lo, hi, rows = L.trajectory_of(case, k)
    y = x[k, ax].copy()
    j = 2 * r * seg + 1                       # the velocity coefficient of that segment: of order 1 m/s
    assert abs(y[j]) > 1e-3
    y[j] *= 1.0 + 1e-6
    prim, stat, comp = kkt_certificate_rows(r, M, T, y, wp[:, ax], bc[0, :, ax], bc[1, :, ax], lo[1:M, ax], hi[1:M, ax], L.certificate_rows(rows, ax))
    assert prim >= PRIM or stat >= STAT or comp >= COMP, (prim, stat, comp)
