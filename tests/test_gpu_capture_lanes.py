"""GPU: replays laid out by conflict (csrc/uavqp_capture.h: lay_out) -- a solve follows the solve it conflicts with into that solve's
lane, so a rotation over any number of buffer sets replays as ONE stage of chains, and the lanes meet only in front of a solve with
predecessors in two of them.  The comparison is that of tests/test_gpu_capture_overlap.py (its helpers are used as they are): every buffer
BITWISE against the same calls made eagerly in the same order on fresh buffers, on the first replay and on the second.  Which lanes and
stages the layout draws is pinned by tests/test_capture_lanes.py; here only results count."""
import numpy as np
import pytest

import test_gpu_capture_overlap as O

pytestmark = pytest.mark.gpu

SHAPES = O.SHAPES   # (4, 8, 64), (4, 8, 37), (3, 5, 64): several tile-4 waves, a shifted partial tile, the odd-M path
BAD = (5, 1)        # (trajectory, segment) of the non-positive duration in buffer set 0


def _rotation(r, M, n, sets, solves):
    """`solves` solves over `sets` buffer sets that share one status array; set 0 carries a non-positive duration."""
    def make():
        bufs = {"st": O._fill(n, "i")}
        for s in range(sets):
            wp, T, bc = O._inputs(r, M, n, seed=200 + s, bad=BAD if s == 0 else None)
            bufs.update({f"wp{s}": O._dev(wp), f"T{s}": O._dev(T), f"bc{s}": O._dev(bc), f"out{s}": O._fill(O._n_coeff(r, M, n), "d")})
        return bufs

    def enqueue(ctx, b):
        for i in range(solves):
            s = i % sets
            ctx.solve_batch_device(r, n, M, M, None, b[f"wp{s}"], b[f"T{s}"], b[f"bc{s}"], b[f"out{s}"], b["st"])

    return make, enqueue


def _check_rotation(ctx, r, M, n, sets, solves):
    import uav_motion_planning_amd as U
    make, enqueue = _rotation(r, M, n, sets, solves)
    eager = O._check(ctx, make, enqueue)
    st = eager["st"].cpu().numpy()
    last = (solves - 1) % sets                                  # the array holds the last writer's values
    if last == 0:
        assert st[BAD[0]] == U.UAVQP_INVALID_INPUT and np.all(np.delete(st, BAD[0]) == U.UAVQP_SOLVED)
    else:
        assert np.all(st == U.UAVQP_SOLVED)
    for s in range(1, sets):
        assert not np.any(O._bits(eager[f"out{s}"]) == np.float64(O.COEFF_FILL).view(np.int64))


@pytest.mark.parametrize("r,M,n", SHAPES)
@pytest.mark.parametrize("lanes", [None, "2", "3", "4"])
def test_rotation_over_five_sets_is_one_stage(gpu_ctx, monkeypatch, r, M, n, lanes):
    """21 solves over 5 sets, a lane for every launch the stage has (UAVQP_CAPTURE_LANE_NODES=1): one stage of 2 (the default), 3 or 4 chains,
    the last solve -- set 0, with the invalid trajectory -- is the one whose statuses stay."""
    monkeypatch.setenv("UAVQP_CAPTURE_LANE_NODES", "1")
    if lanes is None:
        monkeypatch.delenv("UAVQP_CAPTURE_LANES", raising=False)
    else:
        monkeypatch.setenv("UAVQP_CAPTURE_LANES", lanes)
    _check_rotation(gpu_ctx, r, M, n, sets=5, solves=21)


@pytest.mark.parametrize("r,M,n", SHAPES)
def test_seventy_solves_at_the_default_knobs(gpu_ctx, monkeypatch, r, M, n):
    """70 launches at 16 launches a lane: long chains as in the benchmark, two of them by default."""
    monkeypatch.delenv("UAVQP_CAPTURE_LANE_NODES", raising=False)
    monkeypatch.delenv("UAVQP_CAPTURE_LANES", raising=False)
    _check_rotation(gpu_ctx, r, M, n, sets=5, solves=70)


@pytest.mark.parametrize("r,M,n", SHAPES)
def test_seventy_solves_on_four_lanes(gpu_ctx, monkeypatch, r, M, n):
    """The same with UAVQP_CAPTURE_LANES=4: lanes_that_pay(70, 4) == 4, four long chains."""
    monkeypatch.delenv("UAVQP_CAPTURE_LANE_NODES", raising=False)
    monkeypatch.setenv("UAVQP_CAPTURE_LANES", "4")
    _check_rotation(gpu_ctx, r, M, n, sets=5, solves=70)


@pytest.mark.parametrize("r,M,n", SHAPES)
def test_lanes_meet_in_front_of_a_solve_with_inputs_from_two_of_them(gpu_ctx, monkeypatch, r, M, n):
    """Solves 0..3 go to four lanes; solve 4 takes its durations from solve 0's coefficients (many are not positive: invalid input) and its
    boundary values from solve 2's; four more independent solves follow it."""
    import uav_motion_planning_amd as U
    monkeypatch.setenv("UAVQP_CAPTURE_LANE_NODES", "1")
    monkeypatch.setenv("UAVQP_CAPTURE_LANES", "4")
    n_bc = n * 2 * (r - 1) * 3

    def make():
        bufs = {}
        for s in range(9):
            wp, T, bc = O._inputs(r, M, n, seed=300 + s)
            bufs.update({f"wp{s}": O._dev(wp), f"T{s}": O._dev(T), f"bc{s}": O._dev(bc), f"out{s}": O._fill(O._n_coeff(r, M, n), "d"),
                         f"st{s}": O._fill(n, "i")})
        return bufs

    def enqueue(ctx, b):
        for s in range(9):
            T, bc = b[f"T{s}"], b[f"bc{s}"]
            if s == 4:
                T, bc = b["out0"][2:2 + n * M], b["out2"][4:4 + n_bc]
            ctx.solve_batch_device(r, n, M, M, None, b[f"wp{s}"], T, bc, b[f"out{s}"], b[f"st{s}"])

    eager = O._check(gpu_ctx, make, enqueue)
    st4 = eager["st4"].cpu().numpy()
    assert np.any(st4 == U.UAVQP_INVALID_INPUT) and not np.any(st4 == O.STATUS_FILL)
    for s in (0, 1, 2, 3, 5, 6, 7, 8):
        assert np.all(eager[f"st{s}"].cpu().numpy() == U.UAVQP_SOLVED)


@pytest.mark.parametrize("r,M,n", SHAPES)
@pytest.mark.parametrize("lanes", [None, "2", "3", "4"])
def test_rotation_whose_solves_feed_the_next_round_of_their_set(gpu_ctx, monkeypatch, r, M, n, lanes):
    """21 solves over 5 sets with two coefficient arrays per set: round j of set s takes its boundary values from what round j - 1 of the
    same set wrote and writes the array round j - 1 took its own from.  Every solve of a set depends on the one before it (read-after-write
    and write-after-read), so a solve that did not follow its predecessor in that one's lane would compute other bytes."""
    import uav_motion_planning_amd as U
    monkeypatch.setenv("UAVQP_CAPTURE_LANE_NODES", "1")
    if lanes is None:
        monkeypatch.delenv("UAVQP_CAPTURE_LANES", raising=False)
    else:
        monkeypatch.setenv("UAVQP_CAPTURE_LANES", lanes)
    sets, solves = 5, 21
    n_bc = n * 2 * (r - 1) * 3

    def make():
        bufs = {}
        for s in range(sets):
            wp, T, bc = O._inputs(r, M, n, seed=400 + s)
            bufs.update({f"wp{s}": O._dev(wp), f"T{s}": O._dev(T), f"bc{s}": O._dev(bc), f"st{s}": O._fill(n, "i"),
                         f"out{s}a": O._fill(O._n_coeff(r, M, n), "d"), f"out{s}b": O._fill(O._n_coeff(r, M, n), "d")})
        return bufs

    def enqueue(ctx, b):
        for i in range(solves):
            s, j = i % sets, i // sets
            dst, src = (b[f"out{s}a"], b[f"out{s}b"]) if j % 2 == 0 else (b[f"out{s}b"], b[f"out{s}a"])
            bc = b[f"bc{s}"] if j == 0 else src[4:4 + n_bc]
            ctx.solve_batch_device(r, n, M, M, None, b[f"wp{s}"], b[f"T{s}"], bc, dst, b[f"st{s}"])

    eager = O._check(gpu_ctx, make, enqueue)
    fill = np.float64(O.COEFF_FILL).view(np.int64)
    for s in range(sets):
        assert np.all(eager[f"st{s}"].cpu().numpy() == U.UAVQP_SOLVED)
        a, b_ = O._bits(eager[f"out{s}a"]), O._bits(eager[f"out{s}b"])
        assert not np.any(a == fill) and not np.any(b_ == fill) and not np.array_equal(a, b_)    # every round computed something else
