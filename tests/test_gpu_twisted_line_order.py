"""GPU: the 16-lanes-per-trajectory shape of the register-resident solve (variant 4, tiles of 4) emits adjacent segments from the two
lane pairs of a side in the same step and copies whole 128-byte lines out of staging rows ordered by address (csrc/qp_twisted_map.h;
the map itself is checked on the CPU by tests/test_twisted_map.py).  Here: every segment lands at its own place.  The coefficient
rows are pre-filled with a sentinel and every boundary derivative is non-zero, so a segment stored at another segment's place, or
left out, cannot agree with the oracle to the 1e-9 of tests/test_gpu_parity.py (relative, per trajectory, 'distance' durations).
Shapes: both parities of M, one and two emission steps (H = 1: M <= 4, H = 2: M = 5, 7, 8; H = 4: M = 16), both chunk sizes
(r = 4: 64 bytes, r = 3: 48 bytes); batches of one whole tile (4: the one-tile instantiation), a shifted last tile (5), less
than a tile (3: guarded loads, descriptor shorter than a tile) and three tiles (12)."""
import numpy as np
import pytest

from uav_motion_planning_amd import UAVQP_INVALID_INPUT, UAVQP_SOLVED
from uav_motion_planning_amd import workloads as W

pytestmark = pytest.mark.gpu

SHAPES = [(4, 8), (4, 7), (4, 3), (4, 2), (3, 16), (3, 5), (3, 2)]
SIZES = [4, 5, 3, 12]
VARIANT = 4
NMAX = max(SIZES)
SENTINEL = 12345.678
_cache = {}


def _base(r, M):
    if (r, M) not in _cache:
        b = W.uniform_batch(500 + 10 * r + M, NMAX, M, r, time_mode="distance")
        b["bc"] = np.random.default_rng(11 * r + M).uniform(-2.0, 2.0, size=b["bc"].shape)    # every boundary derivative non-zero
        assert np.all(b["bc"] != 0.0)
        _cache[(r, M)] = b
    return _cache[(r, M)]


def _inputs(r, M, n):
    b = _base(r, M)
    return b["waypoints"][:n].copy(), b["times"][:n].copy(), b["bc"][:n].copy()


def _solve(ctx, r, M, wp, T, bc, status=True):
    """Device entry on fresh tensors; the coefficient rows are pre-filled with SENTINEL, the statuses with -77."""
    import torch
    dev = torch.device("cuda", 0)
    n = T.shape[0]

    def put(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(dev)

    d_wp, d_T, d_bc = put(wp), put(T), put(bc)
    d_c = put(np.full(n * 3 * M * 2 * r, SENTINEL))
    d_st = torch.full((n,), -77, dtype=torch.int32, device=dev) if status else None
    torch.cuda.synchronize()                     # the fills above ran on torch's stream, the solve runs on the ctx's
    ctx.set_variant(VARIANT)
    try:
        ctx.solve_batch_device(r, n, M, M, None, d_wp, d_T, d_bc, d_c, d_st)
        ctx.synchronize()
    finally:
        ctx.set_variant(0)
    torch.cuda.synchronize()
    return d_c.cpu().numpy().reshape(n, -1), (d_st.cpu().numpy() if status else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def exact(oracle):
    """oracle.solve_exact_batch of the NMAX trajectories of a shape, computed once and shared."""
    memo = {}

    def get(r, M):
        if (r, M) not in memo:
            wp, T, bc = _inputs(r, M, NMAX)
            so = (np.arange(NMAX + 1) * M).astype(np.int32)
            ref, st = oracle.solve_exact_batch(r, so, wp, T, bc)
            assert np.all(st == 0)
            ref = ref.reshape(NMAX, -1)
            ref.setflags(write=False)
            memo[(r, M)] = ref
        return memo[(r, M)]
    return get


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("r,M", SHAPES)
def test_every_segment_lands_at_its_place(gpu_ctx, exact, r, M, n):
    ref = exact(r, M)[:n]
    wp, T, bc = _inputs(r, M, n)
    got, st = _solve(gpu_ctx, r, M, wp, T, bc)
    assert np.all(st == UAVQP_SOLVED), st
    assert not np.any(got == SENTINEL), "a piece of a solved row was never written"
    err = np.max(np.abs(got - ref), axis=1) / np.maximum(np.max(np.abs(ref), axis=1), 1e-300)
    print(f"r {r} M {M} n {n}: max rel err {err.max():.3e}")
    assert err.max() < 1e-9, f"max rel err {err.max():.3e}"
    # per segment and axis too: a chunk at a wrong place is wrong by the size of the coefficients themselves
    g4, r4 = got.reshape(n, 3, M, 2 * r), ref.reshape(n, 3, M, 2 * r)
    seg_err = np.max(np.abs(g4 - r4), axis=3) / np.max(np.abs(r4), axis=(1, 2, 3))[:, None, None]
    assert seg_err.max() < 1e-9, np.argwhere(seg_err >= 1e-9)[:8]

    without, none = _solve(gpu_ctx, r, M, wp, T, bc, status=False)
    assert none is None
    assert np.array_equal(_bits(got), _bits(without)), "status = None changed the coefficients"

    # one invalid duration, once in each half: the trajectory's rows stay untouched, its neighbours do not change
    bad_traj = n // 2
    others = np.delete(np.arange(n), bad_traj)
    for seg, bad in ((0, 0.0), (M - 1, np.nan)):
        Tb = T.copy()
        Tb[bad_traj, seg] = bad
        gb, sb = _solve(gpu_ctx, r, M, wp, Tb, bc)
        assert sb[bad_traj] == UAVQP_INVALID_INPUT and np.all(sb[others] == UAVQP_SOLVED), (seg, sb)
        assert np.all(gb[bad_traj] == SENTINEL), (seg, "coefficient rows of an invalid trajectory were written")
        assert np.array_equal(_bits(gb[others]), _bits(got[others])), (seg, "a neighbour of an invalid trajectory changed")
