"""GPU: with UAVQP_CAPTURE_FUSE not set, a launch of a replay carries as many independent solves of one shape as a budget of waves
holds in the kernel their group runs (csrc/uavqp_capture.h: fuse_cap, member_waves; UAVQP_CAPTURE_FUSE_WAVES), between 2 and 8.  The
comparison is that of tests/test_gpu_capture_overlap.py (its helpers are used as they are): every buffer BITWISE against the same calls
made eagerly in the same order on fresh buffers, on the first replay and on the second.  Which solves share a launch is not taken from a
profiler: the solves a test enqueues are handed, with the addresses of the captured buffers, to tests/cpp/capture_fuse_waves_plan.cpp --
the host rules themselves, compiled without the HIP runtime.

The smallest shapes at which a cap can go wrong, all at tile 4 (a wave of the captured launch holds four trajectories):

    n    kernel of a group        waves per member    cap at a budget of 4    of 8    default
    8    eight per wave           1                   4                       8       8
    16   eight per wave           2                   2                       4       --
    12   16-lane group kernel     3                   2 (the lower bound)     2       --

over rotations of 9 solves over 5 buffer sets and 17 over 9, so that on one lane a group can reach 4 and 8 members before the lane meets
its own set again."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_gpu_capture_overlap as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uav_motion_planning_amd", "csrc")
RM = [(4, 8), (3, 5)]
BAD = (2, 1)        # (trajectory, segment) of the non-positive duration in buffer set 0
ROTATIONS = [(9, 5), (17, 9)]      # (solves, buffer sets)
# (n, UAVQP_CAPTURE_FUSE_WAVES or None = not set, the cap the table above gives)
CAPS = [(8, 4, 4), (8, 8, 8), (8, None, 8), (16, 4, 2), (16, 8, 4), (12, 4, 2), (12, 8, 2)]


def _cap(n, budget):
    """The table, worked out here: min(8, max(2, budget // waves per member))."""
    waves = n // 8 if n % 8 == 0 else n // 4
    return min(8, max(2, budget // waves))


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """plan(solves, lanes, budget) -> the launches of the replay, each (cap of its first solve, list of indices into `solves`)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    import torch
    exe = str(tmp_path_factory.mktemp("fuse_waves_plan") / "capture_fuse_waves_plan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "capture_fuse_waves_plan.cpp"), "-o", exe])
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count

    def plan(solves, lanes, budget):
        text = f"{lanes} 1 {'-' if budget is None else budget} {num_cus} {len(solves)}\n" + "".join(" ".join(str(int(v)) for v in s) + "\n" for s in solves)
        out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        launches = [(int(line.split()[2]), [int(v) for v in line.split()[3:]]) for line in out.splitlines()]
        assert sorted(k for _, g in launches for k in g) == list(range(len(solves)))
        return launches
    return plan


def _knobs(monkeypatch, lanes, budget):
    monkeypatch.delenv("UAVQP_CAPTURE_FUSE", raising=False)  # no named count: the budget decides
    monkeypatch.setenv("UAVQP_CAPTURE_LANE_NODES", "1")     # small captures are rebuilt
    monkeypatch.setenv("UAVQP_CAPTURE_LANES", str(lanes))
    if budget is None:
        monkeypatch.delenv("UAVQP_CAPTURE_FUSE_WAVES", raising=False)
    else:
        monkeypatch.setenv("UAVQP_CAPTURE_FUSE_WAVES", str(budget))


class Calls:
    """enqueue() for O._check that also keeps what the LAST run (the captured one) passed: the records of the capture.
    calls: (r, M, n, buffer-set name) per solve; a set named in `no_status` is solved without a status array."""

    def __init__(self, calls, no_status=()):
        self.calls, self.no_status, self.solves = calls, no_status, []

    def __call__(self, ctx, b):
        self.solves = []
        for r, M, n, s in self.calls:
            status = None if s in self.no_status else b[f"st{s}"]
            ctx.solve_batch_device(r, n, M, M, None, b[f"wp{s}"], b[f"T{s}"], b[f"bc{s}"], b[f"out{s}"], status)
            self.solves.append((r, M, 4, n, b[f"wp{s}"].data_ptr(), b[f"T{s}"].data_ptr(), b[f"bc{s}"].data_ptr(), b[f"out{s}"].data_ptr(),
                                0 if status is None else status.data_ptr()))


def _set(bufs, s, r, M, n, seed, bad=None, status=True):
    wp, T, bc = O._inputs(r, M, n, seed=seed, bad=bad)
    bufs.update({f"wp{s}": O._dev(wp), f"T{s}": O._dev(T), f"bc{s}": O._dev(bc), f"out{s}": O._fill(O._n_coeff(r, M, n), "d")})
    if status:
        bufs[f"st{s}"] = O._fill(n, "i")


def _sentinels(t):
    return O._bits(t) == np.float64(O.COEFF_FILL).view(np.int64)


def _statuses_and_rows(eager, sets, r, M, bad_set, no_status):
    """The invalid duration of `bad_set` shows in that set's statuses and nowhere else; its trajectory's rows are the only ones never
    written; a set in `no_status` has no status array at all.  sets: {name: n}."""
    import uav_motion_planning_amd as U
    per_traj = 3 * 2 * r * M
    for s, n in sets.items():
        left = _sentinels(eager[f"out{s}"]).reshape(n, per_traj)
        if s in no_status:
            assert f"st{s}" not in eager
        st = None if s in no_status else eager[f"st{s}"].cpu().numpy()
        if s == bad_set:
            assert st[BAD[0]] == U.UAVQP_INVALID_INPUT and np.all(np.delete(st, BAD[0]) == U.UAVQP_SOLVED)
            assert np.all(left[BAD[0]]) and not np.any(np.delete(left, BAD[0], axis=0))
        else:
            assert st is None or np.all(st == U.UAVQP_SOLVED)
            assert not np.any(left)


def _rotation(ctx, planner, r, M, n, lanes, budget, cap, solves, sets):
    """`solves` solves over `sets` buffer sets, each with a status array of its own except set 1, which has none; set 0 carries a
    non-positive duration."""
    def make():
        bufs = {}
        for s in range(sets):
            _set(bufs, s, r, M, n, seed=1500 + s, bad=BAD if s == 0 else None, status=s != 1)
        return bufs

    enqueue = Calls([(r, M, n, i % sets) for i in range(solves)], no_status=(1,))
    eager = O._check(ctx, make, enqueue)                               # bitwise, both replays
    launches = planner(enqueue.solves, lanes, budget)
    sizes = sorted(len(g) for _, g in launches)
    print(f"r={r} M={M} n={n} lanes={lanes} budget={budget}: {solves} solves over {sets} sets -> launches {launches}")
    assert all(c == cap for c, _ in launches) and sizes[-1] <= cap
    if lanes == 1:
        assert sizes[-1] == min(cap, sets, solves)                     # a lane meets a set again after `sets` solves
    else:
        assert sizes[-1] >= 2                                          # the replay checked above ran a group kernel
    for _, g in launches:
        assert len({i % sets for i in g}) == len(g)                    # no launch carries a buffer set twice
    _statuses_and_rows(eager, {s: n for s in range(min(sets, solves))}, r, M, 0, (1,))


@pytest.mark.parametrize("r,M", RM)
@pytest.mark.parametrize("n,budget,cap", CAPS)
@pytest.mark.parametrize("lanes", [1, 2])
def test_rotations_under_a_budget_of_waves(gpu_ctx, planner, monkeypatch, r, M, n, budget, cap, lanes):
    if budget is not None:
        assert cap == _cap(n, budget)
    _knobs(monkeypatch, lanes, budget)
    for solves, sets in ROTATIONS:
        _rotation(gpu_ctx, planner, r, M, n, lanes, budget, cap, solves, sets)


@pytest.mark.parametrize("r,M", RM)
@pytest.mark.parametrize("budget", [4, 8])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("pattern", ["runs", "alternating"])
def test_two_caps_in_one_capture(gpu_ctx, planner, monkeypatch, r, M, budget, lanes, pattern):
    """Solves of n = 8 (sets 0..8) and of n = 16 (sets 9..17) in one capture, every set solved once: in runs of five and four of a
    kind -- on one lane a run is cut by its own shape's cap, 4 / 2 at a budget of 4 and 8 / 4 at 8 -- and alternating, where on one
    lane every solve is a launch (the shape changes each time) and two lanes get one shape each."""
    _knobs(monkeypatch, lanes, budget)
    n_of = {s: 8 if s < 9 else 16 for s in range(18)}
    if pattern == "runs":
        order = [0, 1, 2, 3, 4, 9, 10, 11, 12, 13, 5, 6, 7, 8, 14, 15, 16, 17]
    else:
        order = [s for pair in zip(range(9), range(9, 18)) for s in pair]

    def make():
        bufs = {}
        for s in range(18):
            _set(bufs, s, r, M, n_of[s], seed=1600 + s, bad=BAD if s == 0 else None, status=s != 1)
        return bufs

    enqueue = Calls([(r, M, n_of[s], s) for s in order], no_status=(1,))
    eager = O._check(gpu_ctx, make, enqueue)
    launches = planner(enqueue.solves, lanes, budget)
    print(f"r={r} M={M} budget={budget} lanes={lanes} {pattern}: launches {launches}")
    largest = {8: 0, 16: 0}
    for cap, g in launches:
        ns = {n_of[order[k]] for k in g}
        assert len(ns) == 1                                            # a launch is of one shape
        n = ns.pop()
        assert cap == _cap(n, budget) and len(g) <= cap
        largest[n] = max(largest[n], len(g))
    if lanes == 1 and pattern == "runs":
        assert largest == {8: min(_cap(8, budget), 5), 16: min(_cap(16, budget), 5)}
        assert sorted(len(g) for _, g in launches) == ([1, 1, 2, 2, 2, 2, 4, 4] if budget == 4 else [1, 4, 4, 4, 5])
    elif lanes == 1:
        assert largest == {8: 1, 16: 1}
    elif pattern == "alternating":
        assert largest == {8: _cap(8, budget), 16: _cap(16, budget)}   # lane 0 has the nine solves of n = 8, lane 1 those of n = 16
    _statuses_and_rows(eager, n_of, r, M, 0, (1,))
