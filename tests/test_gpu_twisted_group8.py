"""GPU: a group of independent tile-4 solves over a whole number of eights is replayed by solve_twisted_group8_kernel (csrc/qp_twisted.h):
eight trajectories per wave, the elimination once per (trajectory, axis, side) instead of once per lane pair of the 16-lane shape, both
segments of a 16-lane step emitted by the one pair.  The per-segment arithmetic is the 16-lane kernel's, so the comparison is that of
tests/test_gpu_capture_overlap.py (its helpers are used as they are): every buffer BITWISE against the same calls made eagerly in the same
order on fresh buffers, on the first replay and on the second.

Which kernel a capture's groups ran is not taken from a profiler: the captured solves go to tests/cpp/capture_fuse_plan.cpp (the groups
the host draws) and each group to tests/cpp/test_twisted_group8_map.cpp `choose` (csrc/uavqp_capture.h: group_kernel_choice -- the
function uavqp_capture_end itself asks).  n = 8 and 24 put the new kernel on one wave and on three; n = 12 is no whole number of eights and
keeps the 16-lane group kernel; (4, 7) has no group kernel at all and replays one launch per solve.

Every buffer set has boundary derivatives that are not zero at both ends; set 0 has a non-positive duration in trajectory 2 and one in
trajectory 5 of a wave -- one in each half of the eight -- and set 1 has no status array."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_gpu_capture_overlap as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uav_motion_planning_amd", "csrc")
RM = [(4, 8), (4, 7), (4, 2), (3, 5), (3, 16)]
# csrc/kernel_instances.h: UAVQP_GROUP8_PAIRS* -- (4, 7) is not in the tile-4 group lists (182 VGPRs at 16 lanes), so it has neither kernel
HAS_GROUP8 = {(4, 8): True, (4, 7): False, (4, 2): True, (3, 5): True, (3, 16): True}
ROTATIONS = [(2, 3), (6, 3), (9, 4)]     # (solves, buffer sets)
AS_CAPTURED, OWN_TILE, EIGHT_PER_WAVE = 0, 1, 2


def _cxx(tmp, name, source):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", source), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def host_rules(tmp_path_factory):
    """(plan, choose): plan(solves, lanes, F) -> the launches of the replay as lists of indices into `solves`; choose(members, r, M, tile, n) ->
    the kernel of such a group's node."""
    import torch
    tmp = tmp_path_factory.mktemp("group8_rules")
    plan_exe, choose_exe = _cxx(tmp, "capture_fuse_plan", "capture_fuse_plan.cpp"), _cxx(tmp, "group8_choose", "test_twisted_group8_map.cpp")
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count

    def plan(solves, lanes, F):
        text = f"{lanes} 1 {F} {num_cus} {len(solves)}\n" + "".join(" ".join(str(int(v)) for v in s) + "\n" for s in solves)
        out = subprocess.run([plan_exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        launches = [[int(v) for v in line.split()[2:]] for line in out.splitlines()]
        assert sorted(k for g in launches for k in g) == list(range(len(solves)))
        return launches

    memo = {}

    def choose(members, r, M, tile, n):
        key = (members, r, M, tile, n)
        if key not in memo:
            memo[key] = int(subprocess.run([choose_exe, "choose"] + [str(v) for v in key] + [str(num_cus)], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout)
        return memo[key]
    return plan, choose


def _bad(n, M):
    """(trajectory, segment) of the non-positive durations of set 0: trajectories 2 and 5 of the last wave of eight."""
    base = (n // 8 - 1) * 8 if n >= 8 else 0
    return [(base + 2, min(1, M - 1)), (base + 5, 0)]


_HOST = {}


def _host_inputs(r, M, n, seed, bad):
    """Inputs of one set, computed once per (shape, seed) and never changed: the workload's paths and durations, every boundary derivative of
    both ends drawn from +-[0.1, 0.6] (none is zero)."""
    key = (r, M, n, seed, bad)
    if key not in _HOST:
        wp, T, bc = O._inputs(r, M, n, seed=seed)
        rng = np.random.default_rng(9000 + seed)
        bc = (rng.uniform(0.1, 0.6, size=bc.shape) * rng.choice([-1.0, 1.0], size=bc.shape)).astype(np.float64)
        T = T.copy().reshape(n, M)
        for t, s in bad:
            T[t, s] = -0.5
        _HOST[key] = (wp, T.reshape(-1), bc)
    return _HOST[key]


def _make(r, M, n, sets):
    def make():
        bufs = {}
        for s in range(sets):
            wp, T, bc = _host_inputs(r, M, n, 900 + s, tuple(_bad(n, M)) if s == 0 else ())
            bufs.update({f"wp{s}": O._dev(wp), f"T{s}": O._dev(T), f"bc{s}": O._dev(bc), f"out{s}": O._fill(O._n_coeff(r, M, n), "d")})
            if s != 1:
                bufs[f"st{s}"] = O._fill(n, "i")
        return bufs
    return make


def _sentinels(t):
    return O._bits(t) == np.float64(O.COEFF_FILL).view(np.int64)


def _rotation(ctx, host_rules, r, M, n, lanes, F, solves, sets, has_group=None, has_group8=None, report=None):
    """has_group / has_group8: is (r, M) in the tile-4 group list / the eight-per-wave list (default: HAS_GROUP8 for both -- the two
    lists of csrc/kernel_instances.h are one); report: a dict that receives the launches and their kernels."""
    import uav_motion_planning_amd as U
    plan, choose = host_rules
    has_group8 = HAS_GROUP8[(r, M)] if has_group8 is None else has_group8
    has_group = has_group8 if has_group is None else has_group
    captured = []

    def enqueue(c, b):
        del captured[:]
        for i in range(solves):
            s = i % sets
            status = None if s == 1 else b[f"st{s}"]
            c.solve_batch_device(r, n, M, M, None, b[f"wp{s}"], b[f"T{s}"], b[f"bc{s}"], b[f"out{s}"], status)
            captured.append((r, M, 4, n, b[f"wp{s}"].data_ptr(), b[f"T{s}"].data_ptr(), b[f"bc{s}"].data_ptr(), b[f"out{s}"].data_ptr(),
                             0 if status is None else status.data_ptr()))

    eager = O._check(ctx, _make(r, M, n, sets), enqueue)           # bitwise, both replays
    launches = plan(captured, lanes, F)
    kernels = [choose(len(g), r, M, 4, n) for g in launches]
    print(f"r={r} M={M} n={n} lanes={lanes} F={F}: {solves} solves over {sets} sets -> launches {launches}, kernels {kernels}")
    for g, k in zip(launches, kernels):
        if len(g) == 1:
            assert k == AS_CAPTURED
        elif n % 8 == 0 and has_group8:
            assert k == EIGHT_PER_WAVE
        else:
            assert k == OWN_TILE                                   # n = 12: the 16-lane group kernel, as before
    if report is not None:
        report.update(launches=launches, kernels=kernels)
    if not has_group:
        assert all(len(g) == 1 for g in launches)
    elif lanes == 1:
        assert max(len(g) for g in launches) == min(F, sets, solves)   # a lane meets a set again after `sets` solves
        assert (EIGHT_PER_WAVE in kernels) == (n % 8 == 0 and has_group8)   # the replay checked above ran the new kernel / did not
    elif solves > lanes:
        assert max(len(g) for g in launches) >= 2 and (EIGHT_PER_WAVE in kernels) == (n % 8 == 0 and has_group8)
    # the invalid durations of set 0 show in set 0's statuses and nowhere else; their trajectories' rows are the only ones never written
    per_traj = 3 * 2 * r * M
    bad = [t for t, _ in _bad(n, M)]
    for s in range(min(sets, solves)):
        left = _sentinels(eager[f"out{s}"]).reshape(n, per_traj)
        st = None if s == 1 else eager[f"st{s}"].cpu().numpy()
        if s == 0:
            assert np.all(st[bad] == U.UAVQP_INVALID_INPUT) and np.all(np.delete(st, bad) == U.UAVQP_SOLVED)
            assert np.all(left[bad]) and not np.any(np.delete(left, bad, axis=0))
        else:
            assert st is None or np.all(st == U.UAVQP_SOLVED)
            assert not np.any(left)
    return eager


@pytest.mark.parametrize("r,M", RM)
@pytest.mark.parametrize("n", [8, 24, 12])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("F", [2, 3, 8])
def test_rotations_bitwise_equal_to_eager_order(gpu_ctx, host_rules, monkeypatch, r, M, n, lanes, F):
    monkeypatch.setenv("UAVQP_CAPTURE_LANE_NODES", "1")     # small captures are rebuilt
    monkeypatch.setenv("UAVQP_CAPTURE_LANES", str(lanes))
    monkeypatch.setenv("UAVQP_CAPTURE_FUSE", str(F))
    for solves, sets in ROTATIONS:
        _rotation(gpu_ctx, host_rules, r, M, n, lanes, F, solves, sets)


@pytest.mark.parametrize("r,M", [(4, 8), (3, 5)])
def test_replay_against_the_binary128_oracle(gpu_ctx, host_rules, monkeypatch, r, M):
    """What the new kernel wrote (the eager buffers are bitwise the replayed ones: _check) against the exact minimiser, per valid trajectory."""
    from oracle import oracle
    monkeypatch.setenv("UAVQP_CAPTURE_LANE_NODES", "1")
    monkeypatch.setenv("UAVQP_CAPTURE_LANES", "1")
    monkeypatch.setenv("UAVQP_CAPTURE_FUSE", "8")
    n, solves, sets = 24, 6, 3
    eager = _rotation(gpu_ctx, host_rules, r, M, n, 1, 8, solves, sets)
    so = (np.arange(n + 1) * M).astype(np.int32)
    bad = [t for t, _ in _bad(n, M)]
    for s in range(sets):
        wp, T, bc = _host_inputs(r, M, n, 900 + s, tuple(_bad(n, M)) if s == 0 else ())
        valid = np.array([t for t in range(n) if not (s == 0 and t in bad)])
        Tv = T.reshape(n, M).copy()
        if s == 0:
            Tv[bad] = 1.0                                      # (the oracle is not asked about the invalid trajectories)
        ref, _ = oracle.solve_exact_batch(r, so, wp.reshape(n, M + 1, 3), Tv, bc.reshape(n, 2, r - 1, 3))
        got = eager[f"out{s}"].cpu().numpy().reshape(n, -1)[valid]
        ref = np.asarray(ref).reshape(n, -1)[valid]
        err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
        print(f"r={r} M={M} set {s}: max rel err vs the binary128 oracle {err:.2e}")
        assert err < 1e-9, err
