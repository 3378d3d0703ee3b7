"""GPU: the eight-per-wave kernel at three waves per SIMD, and its own default budget of waves (csrc/qp_twisted_body.h: the copy-out decode
behind the elimination; csrc/uavqp_capture.h: FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT, fuse_budget, group_cap).  The comparison is that of
tests/test_gpu_twisted_group8.py, whose rotation helper is used as it is: every buffer BITWISE against the same calls made eagerly in the
same order on fresh, sentinel-filled buffers, on the first replay and on the second; set 0 has two non-positive durations, set 1 no
status array.

    (4, 8), (3, 16), (4, 6)   the three shapes whose occupancy changed (2 -> 3, 2 -> 3, 3 -> 4 waves per SIMD); (3, 16) is also the one
                              shape whose idle lane pairs no longer write to LDS (qp_twisted.h: TwistedCfg::IDLE_ROWS2)
    n = 8, 24                 one wave per member and three
    UAVQP_CAPTURE_FUSE 2, 8   the smallest group and the largest; one lane and two

and one capture at n = 4096 with both knobs unset: 512 waves per member is the size at which the candidates for the eight-per-wave
kernel's default budget (2048 / 3072 / 4096 waves) give different caps, 4 / 6 / 8 (every n with n / 8 <= 256 waves has 8 members under
any of them).  Which solves share a launch comes from tests/cpp/capture_kernel_budget_plan.cpp -- the host rules themselves, compiled
without the HIP runtime -- and the cap it must show is worked out here from the constant in the header, whatever its value."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_gpu_capture_overlap as O
import test_gpu_twisted_group8 as G
from test_gpu_twisted_group8 import host_rules  # noqa: F401  (the module-scoped fixture: plan for a named count, kernel choice)

pytestmark = pytest.mark.gpu

RM = [(4, 8), (3, 16), (4, 6)]


@pytest.mark.parametrize("r,M", RM)
@pytest.mark.parametrize("n", [8, 24])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("F", [2, 8])
def test_three_wave_shapes_bitwise_equal_to_eager_order(gpu_ctx, host_rules, monkeypatch, r, M, n, lanes, F):  # noqa: F811
    monkeypatch.setenv("UAVQP_CAPTURE_LANE_NODES", "1")     # small captures are rebuilt
    monkeypatch.setenv("UAVQP_CAPTURE_LANES", str(lanes))
    monkeypatch.setenv("UAVQP_CAPTURE_FUSE", str(F))
    report = {}
    G._rotation(gpu_ctx, host_rules, r, M, n, lanes, F, 9, 4, has_group8=True, report=report)
    assert G.EIGHT_PER_WAVE in report["kernels"]


def _constant(name):
    text = open(os.path.join(G.CSRC, "uavqp_capture.h")).read()
    return int(re.search(r"static constexpr int %s = (\d+);" % name, text).group(1))


def test_headline_batch_takes_the_eight_per_wave_budget(gpu_ctx, monkeypatch, tmp_path):
    """17 solves of 4096 x (4, 8) over 9 buffer sets, UAVQP_CAPTURE_FUSE and UAVQP_CAPTURE_FUSE_WAVES not set, everything else at its
    default: 17 launches are one stage on one lane, which meets set 0 again after nine solves, so the first group is as large as the cap."""
    import torch
    from oracle import oracle
    monkeypatch.delenv("UAVQP_CAPTURE_FUSE", raising=False)
    monkeypatch.delenv("UAVQP_CAPTURE_FUSE_WAVES", raising=False)
    monkeypatch.delenv("UAVQP_CAPTURE_LANES", raising=False)
    monkeypatch.delenv("UAVQP_CAPTURE_LANE_NODES", raising=False)
    r, M, n, solves, sets = 4, 8, 4096, 17, 9
    captured = []

    def enqueue(c, b):
        del captured[:]
        for i in range(solves):
            s = i % sets
            status = None if s == 1 else b[f"st{s}"]
            c.solve_batch_device(r, n, M, M, None, b[f"wp{s}"], b[f"T{s}"], b[f"bc{s}"], b[f"out{s}"], status)
            captured.append((r, M, 4, n, b[f"wp{s}"].data_ptr(), b[f"T{s}"].data_ptr(), b[f"bc{s}"].data_ptr(), b[f"out{s}"].data_ptr(),
                             0 if status is None else status.data_ptr()))

    eager = O._check(gpu_ctx, G._make(r, M, n, sets), enqueue)      # every buffer bitwise, both replays

    exe = G._cxx(tmp_path, "capture_kernel_budget_plan", "capture_kernel_budget_plan.cpp")
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    text = f"2 16 - - {num_cus} {solves}\n" + "".join(" ".join(str(int(v)) for v in s) + "\n" for s in captured)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    launches = [(int(line.split()[2]), [int(v) for v in line.split()[3:]]) for line in out.splitlines()]
    assert sorted(k for _, g in launches for k in g) == list(range(solves))
    budget, other = _constant("FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT"), _constant("FUSE_WAVES_DEFAULT")
    cap = min(8, max(2, budget // (n // 8)))
    print(f"budget {budget}: cap {cap} (the budget of the other kernels, {other}, would give {min(8, max(2, other // (n // 8)))}); launches {launches}")
    assert all(c == cap for c, _ in launches)
    assert max(len(g) for _, g in launches) == cap and len(launches[0][1]) == cap
    for _, g in launches:
        assert len({i % sets for i in g}) == len(g)                  # no launch carries a buffer set twice

    import uav_motion_planning_amd as U
    bad = [t for t, _ in G._bad(n, M)]
    for s in range(sets):
        left = G._sentinels(eager[f"out{s}"]).reshape(n, 3 * 2 * r * M)
        st = None if s == 1 else eager[f"st{s}"].cpu().numpy()
        if s == 0:
            assert np.all(st[bad] == U.UAVQP_INVALID_INPUT) and np.all(np.delete(st, bad) == U.UAVQP_SOLVED)
            assert np.all(left[bad]) and not np.any(np.delete(left, bad, axis=0))
        else:
            assert st is None or np.all(st == U.UAVQP_SOLVED)
            assert not np.any(left)

    # one case against the exact minimiser: the first and the last 64 trajectories of set 2 (what the replay wrote is bitwise the eager buffer)
    wp, T, bc = G._host_inputs(r, M, n, 900 + 2, ())
    pick = np.r_[0:64, n - 64:n]
    so = (np.arange(len(pick) + 1) * M).astype(np.int32)
    ref, _ = oracle.solve_exact_batch(r, so, wp.reshape(n, M + 1, 3)[pick], T.reshape(n, M)[pick], bc.reshape(n, 2, r - 1, 3)[pick])
    got = eager["out2"].cpu().numpy().reshape(n, -1)[pick]
    ref = np.asarray(ref).reshape(len(pick), -1)
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    print(f"n = {n}, set 2, {len(pick)} trajectories: max rel err vs the binary128 oracle {err:.2e}")
    assert err < 1e-9, err
