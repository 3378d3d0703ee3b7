"""GPU: independent captured solves of one shape that follow each other in a lane are replayed as ONE launch of the group kernel
(csrc/uavqp_capture.h: fuse_groups; csrc/qp_twisted.h: solve_twisted_group_kernel).  The comparison is that of
tests/test_gpu_capture_overlap.py (its helpers are used as they are): every buffer BITWISE against the same calls made eagerly in the same
order on fresh buffers, on the first replay and on the second.  Whether a capture was fused is not taken from a profiler: the solves a
test enqueues are handed, with the addresses of the captured buffers, to tests/cpp/capture_fuse_plan.cpp -- the host rule itself,
compiled without the HIP runtime -- and the launches it returns are what the test expects of the capture.  Which groups the rule
draws in general is pinned by tests/test_capture_fuse.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_gpu_capture_overlap as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uav_motion_planning_amd", "csrc")
RM = [(4, 8), (4, 2), (3, 5)]
BAD = (2, 1)        # (trajectory, segment) of the non-positive duration in buffer set 0
# (solves, buffer sets) of the rotations: 2 to 9 solves over 3 to 5 sets
ROTATIONS = [(2, 3), (6, 3), (9, 4), (9, 5)]
# shapes with a group kernel (csrc/kernel_instances.h): at tile 8 min-snap with 8 segments has none -- 200 VGPRs, two waves per SIMD
HAS_GROUP = {(4, 8, 4): True, (4, 2, 4): True, (3, 5, 4): True, (4, 8, 8): False, (4, 2, 8): True, (3, 5, 8): True}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """plan(solves, lanes, F) -> the launches of the replay, each a list of indices into `solves`."""
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    import torch
    exe = str(tmp_path_factory.mktemp("fuse_plan") / "capture_fuse_plan")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "capture_fuse_plan.cpp"), "-o", exe])
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count

    def plan(solves, lanes, F):
        text = f"{lanes} 1 {F} {num_cus} {len(solves)}\n" + "".join(" ".join(str(int(v)) for v in s) + "\n" for s in solves)
        out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        launches = [[int(v) for v in line.split()[2:]] for line in out.splitlines()]
        assert sorted(k for g in launches for k in g) == list(range(len(solves)))
        return launches
    return plan


def _knobs(monkeypatch, lanes, F):
    monkeypatch.setenv("UAVQP_CAPTURE_LANE_NODES", "1")     # small captures are rebuilt
    monkeypatch.setenv("UAVQP_CAPTURE_LANES", str(lanes))
    monkeypatch.setenv("UAVQP_CAPTURE_FUSE", str(F))


class Calls:
    """enqueue() for O._check that also keeps what the LAST run (the captured one) passed: the records of the capture."""

    def __init__(self, tile, calls):
        self.tile, self.calls, self.solves = tile, calls, []

    def __call__(self, ctx, b):
        self.solves = []
        for r, M, n, wp, T, bc, out, st in self.calls:
            status = None if st is None else b[st]
            ctx.solve_batch_device(r, n, M, M, None, b[wp], b[T], b[bc], b[out], status)
            self.solves.append((r, M, self.tile, n, b[wp].data_ptr(), b[T].data_ptr(), b[bc].data_ptr(), b[out].data_ptr(),
                                0 if status is None else status.data_ptr()))


def _set(bufs, s, r, M, n, seed, bad=None, status=True):
    wp, T, bc = O._inputs(r, M, n, seed=seed, bad=bad)
    bufs.update({f"wp{s}": O._dev(wp), f"T{s}": O._dev(T), f"bc{s}": O._dev(bc), f"out{s}": O._fill(O._n_coeff(r, M, n), "d")})
    if status:
        bufs[f"st{s}"] = O._fill(n, "i")


def _sentinels(t):
    return O._bits(t) == np.float64(O.COEFF_FILL).view(np.int64)


def _rotation(ctx, planner, r, M, n, tile, lanes, F, solves, sets, has_group=None):
    """`solves` solves over `sets` buffer sets, each with a status array of its own except set 1, which has none; set 0 carries a
    non-positive duration.  has_group: is (r, M) in the group list of this tile (default: HAS_GROUP).  Returns the eager buffers (bitwise
    the replayed ones) and the launches of the replay."""
    import uav_motion_planning_amd as U
    has_group = HAS_GROUP[(r, M, tile)] if has_group is None else has_group

    def make():
        bufs = {}
        for s in range(sets):
            _set(bufs, s, r, M, n, seed=500 + s, bad=BAD if s == 0 else None, status=s != 1)
        return bufs

    enqueue = Calls(tile, [(r, M, n, f"wp{i % sets}", f"T{i % sets}", f"bc{i % sets}", f"out{i % sets}", None if i % sets == 1 else f"st{i % sets}")
                           for i in range(solves)])
    eager = O._check(ctx, make, enqueue)
    launches = planner(enqueue.solves, lanes, F)
    sizes = sorted(len(g) for g in launches)
    print(f"r={r} M={M} n={n} tile={tile} lanes={lanes} F={F}: {solves} solves over {sets} sets -> launches {launches}")
    assert sizes[-1] <= F
    if F == 1 or not has_group:
        assert sizes[-1] == 1
    elif lanes == 1:
        assert sizes[-1] == min(F, sets, solves)                 # a lane meets a set again after `sets` solves
    elif solves > lanes:
        assert sizes[-1] >= 2                                    # the replay checked above ran the group kernel
    for g in launches:
        assert len({i % sets for i in g}) == len(g)              # no launch carries a buffer set twice
    # the invalid duration of set 0 shows in set 0's statuses and nowhere else; its trajectory's rows are the only ones never written
    per_traj = 3 * 2 * r * M
    for s in range(min(sets, solves)):
        left = _sentinels(eager[f"out{s}"]).reshape(n, per_traj)
        st = None if s == 1 else eager[f"st{s}"].cpu().numpy()
        if s == 0:
            assert st[BAD[0]] == U.UAVQP_INVALID_INPUT and np.all(np.delete(st, BAD[0]) == U.UAVQP_SOLVED)
            assert np.all(left[BAD[0]]) and not np.any(np.delete(left, BAD[0], axis=0))
        else:
            assert st is None or np.all(st == U.UAVQP_SOLVED)
            assert not np.any(left)
    return eager, launches


@pytest.mark.parametrize("r,M", RM)
@pytest.mark.parametrize("n", [4, 12])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("F", [1, 2, 3, 8])
def test_rotations_at_tile_4(gpu_ctx, planner, monkeypatch, r, M, n, lanes, F):
    """One wave (n = 4) and three (n = 12) of 16 lanes per trajectory."""
    _knobs(monkeypatch, lanes, F)
    for solves, sets in ROTATIONS:
        _rotation(gpu_ctx, planner, r, M, n, 4, lanes, F, solves, sets)


@pytest.mark.parametrize("r,M", RM)
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("F", [1, 2, 3, 8])
def test_rotations_at_tile_8(planner, monkeypatch, r, M, lanes, F):
    """Variant 8: one wave of 8 lanes per trajectory over 8 trajectories.  (4, 8) has no group kernel at this tile: it replays unfused."""
    import uav_motion_planning_amd as U
    _knobs(monkeypatch, lanes, F)
    with U.Context(0) as ctx:
        ctx.set_variant(8)
        for solves, sets in ROTATIONS:
            _rotation(ctx, planner, r, M, 8, 8, lanes, F, solves, sets)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("F", [2, 8])
def test_min_jerk_and_min_snap_solves_in_one_capture(gpu_ctx, planner, monkeypatch, lanes, F):
    """Runs of two shapes: a group ends where the shape changes."""
    import uav_motion_planning_amd as U
    _knobs(monkeypatch, lanes, F)
    n = 12
    shapes = [(4, 8), (4, 8), (4, 8), (3, 5), (3, 5), (4, 8), (3, 5), (3, 5), (3, 5)]

    def make():
        bufs = {}
        for s, (r, M) in enumerate(shapes):
            _set(bufs, s, r, M, n, seed=600 + s)
        return bufs

    enqueue = Calls(4, [(r, M, n, f"wp{s}", f"T{s}", f"bc{s}", f"out{s}", f"st{s}") for s, (r, M) in enumerate(shapes)])
    eager = O._check(gpu_ctx, make, enqueue)
    launches = planner(enqueue.solves, lanes, F)
    print(f"lanes={lanes} F={F}: launches {launches}")
    assert max(len(g) for g in launches) >= 2
    for g in launches:
        assert len({shapes[k] for k in g}) == 1
    if lanes == 1:
        assert launches == ([[0, 1], [2], [3, 4], [5], [6, 7], [8]] if F == 2 else [[0, 1, 2], [3, 4], [5], [6, 7, 8]])
    for s in range(len(shapes)):
        assert np.all(eager[f"st{s}"].cpu().numpy() == U.UAVQP_SOLVED) and not np.any(_sentinels(eager[f"out{s}"]))


@pytest.mark.parametrize("r,M", RM)
@pytest.mark.parametrize("lanes", [1, 2])
def test_the_same_set_twice_in_a_row_is_not_fused(gpu_ctx, planner, monkeypatch, r, M, lanes):
    """Set 0 is solved twice, the second time with the boundary values read out of the first solve's coefficients: the two are ordered."""
    import uav_motion_planning_amd as U
    _knobs(monkeypatch, lanes, 8)
    n = 12
    n_bc = n * 2 * (r - 1) * 3

    def make():
        bufs = {}
        for s in range(3):
            _set(bufs, s, r, M, n, seed=700 + s)
        bufs["out0b"] = O._fill(O._n_coeff(r, M, n), "d")
        return bufs

    solves = []

    def enqueue(ctx, b):
        del solves[:]
        calls = [(b["wp0"], b["T0"], b["bc0"], b["out0"], b["st0"]), (b["wp0"], b["T0"], b["out0"][4:4 + n_bc], b["out0b"], b["st0"]),
                 (b["wp1"], b["T1"], b["bc1"], b["out1"], b["st1"]), (b["wp2"], b["T2"], b["bc2"], b["out2"], b["st2"])]
        for wp, T, bc, out, st in calls:
            ctx.solve_batch_device(r, n, M, M, None, wp, T, bc, out, st)
            solves.append((r, M, 4, n, wp.data_ptr(), T.data_ptr(), bc.data_ptr(), out.data_ptr(), st.data_ptr()))

    eager = O._check(gpu_ctx, make, enqueue)
    launches = planner(solves, lanes, 8)
    print(f"r={r} M={M} lanes={lanes}: launches {launches}")
    assert not any(0 in g and 1 in g for g in launches) and max(len(g) for g in launches) >= 2
    if lanes == 1:
        assert launches == [[0], [1, 2, 3]]
    assert not np.any(_sentinels(eager["out0b"])) and not np.array_equal(O._bits(eager["out0"]), O._bits(eager["out0b"]))
    assert np.all(eager["st0"].cpu().numpy() == U.UAVQP_SOLVED)


@pytest.mark.parametrize("r,M", RM)
@pytest.mark.parametrize("lanes", [1, 2])
def test_a_batch_that_is_no_whole_number_of_tiles_is_not_fused(gpu_ctx, planner, monkeypatch, r, M, lanes):
    """n = 6 at tile 4: a shifted partial tile, the kernel with the tile loop -- every solve stays a launch of its own."""
    import uav_motion_planning_amd as U
    _knobs(monkeypatch, lanes, 8)

    def make():
        bufs = {}
        for s in range(3):
            _set(bufs, s, r, M, 6, seed=800 + s)
        return bufs

    enqueue = Calls(4, [(r, M, 6, f"wp{i % 3}", f"T{i % 3}", f"bc{i % 3}", f"out{i % 3}", f"st{i % 3}") for i in range(6)])
    eager = O._check(gpu_ctx, make, enqueue)
    launches = planner(enqueue.solves, lanes, 8)
    assert all(len(g) == 1 for g in launches), launches
    for s in range(3):
        assert np.all(eager[f"st{s}"].cpu().numpy() == U.UAVQP_SOLVED) and not np.any(_sentinels(eager[f"out{s}"]))
