"""GPU: every compiled instance of the register-resident solve (csrc/qp_twisted.h, qp_twisted_body.h) against the binary128 oracle.
csrc/kernel_instances.h compiles the solve once per shape (r, M) and tile shape -- the general kernel at tiles 4 / 8 / 16 / 32, the
one-whole-tile-per-wave kernel (ONE) at tiles 4 and 8, the group kernels at tiles 4 and 8 and the group kernel with eight trajectories
per wave -- each instance unrolled and register-allocated on its own.  The halves (mL = (M + 1) / 2, mR = M / 2), the fill of the last
emission chunk and, at tile 32, whether the staging rows alias the input buffer (ALIAS below) differ from shape to shape, so every shape
of the lists is run; the lists are read from the header (tests/twisted_instances.py): a shape added there is covered here.

Inputs, helpers and the tolerance are those of tests/test_gpu_twisted_one_tile.py: 97 distinct base trajectories per shape with
'distance' durations and non-zero boundary derivatives, larger batches repeat them by index % 97, coefficient rows are pre-filled with a
sentinel and statuses with -77; 1e-9 relative to max|coeff| per trajectory.  The exact minimisers of the 97 are computed once per shape.
The group kernels are reached through capture and replay with the drivers of tests/test_gpu_twisted_group8.py (tile 4) and
tests/test_gpu_capture_fuse.py (tile 8), which require replay bitwise equal to eager and take the kernel of each launch from the host
rules; the eager buffers are then held against the oracle.  Every comparison prints its maximum error (docs/measurement_log.md)."""
import numpy as np
import pytest

import test_gpu_capture_fuse as F
import test_gpu_capture_overlap as O
import test_gpu_twisted_group8 as G
import twisted_instances as TI
from test_gpu_twisted_group8 import host_rules      # noqa: F401  (fixture)
from test_gpu_twisted_one_tile import BASE, SENTINEL, _bits, _cus, _inputs, _rel_err, _solve
from uav_motion_planning_amd import UAVQP_INVALID_INPUT, UAVQP_SOLVED

pytestmark = pytest.mark.gpu

TOL = 1e-9
# TwistedCfg::ALIAS: tests/test_twisted_instances.py recomputes the set from qp_twisted.h and fails if it is no longer this one
ALIAS = {(3, 10, 32), (3, 12, 32), (3, 16, 32)}
assert ALIAS <= {(r, M, tile) for r, M in TI.TWISTED for tile in TI.TILES}, "an ALIAS instance is not among the instances run below"
NO_GROUP = {tile: [p for p in TI.TWISTED if p not in TI.GROUP[tile]] for tile in (4, 8)}
_SENTINEL_BITS = np.float64(SENTINEL).view(np.uint64)


def _ids(pairs):
    return [f"r{r}-M{M}" for r, M in pairs]


@pytest.fixture(scope="module")
def exact(oracle):
    """oracle.solve_exact_batch of the 97 base trajectories of a shape, computed once and shared, read-only."""
    memo = {}

    def get(r, M):
        if (r, M) not in memo:
            wp, T, bc = _inputs(r, M, BASE)
            ref, st = oracle.solve_exact_batch(r, (np.arange(BASE + 1) * M).astype(np.int32), wp, T, bc)
            assert np.all(st == 0)
            ref = ref.reshape(BASE, -1)
            ref.setflags(write=False)
            memo[(r, M)] = ref
        return memo[(r, M)]
    return get


def _written(got):
    """Per trajectory: (is every word of the row still the sentinel, is any)."""
    left = _bits(got) == _SENTINEL_BITS
    return left.all(axis=1), left.any(axis=1)


def _check_batch(ctx, ref, r, M, variant, n, first_bad, nan_bad, status=True):
    """One batch on the general path with a non-positive duration in trajectory first_bad (a segment of the reversed half) and a NaN
    duration in trajectory nan_bad (a segment of the forward half).  Returns the maximum relative error of the valid rows."""
    wp, T, bc = _inputs(r, M, n)
    T[first_bad, M - 1] = -0.5
    T[nan_bad, 0] = np.nan
    got, st = _solve(ctx, r, M, variant, wp, T, bc, status=status)
    bad = np.array(sorted({first_bad, nan_bad}))
    valid = np.ones(n, dtype=bool)
    valid[bad] = False
    if status:
        assert np.all(st[bad] == UAVQP_INVALID_INPUT), (n, st[bad])
        wrong = np.flatnonzero(valid & (st != UAVQP_SOLVED))
        assert wrong.size == 0, (n, wrong[:8], st[wrong[:8]])
    else:
        assert st is None
    untouched, any_left = _written(got)
    assert np.all(untouched[bad]), (n, "coefficient rows of an invalid trajectory were written")
    stale = np.flatnonzero(valid & any_left)
    assert stale.size == 0, (n, "rows not fully written", stale[:8])
    idx = np.flatnonzero(valid)
    err = _rel_err(got[idx], ref[idx % BASE])
    worst = int(idx[np.argmax(err)])
    print(f"general tile {variant} r {r} M {M} n {n}{'' if status else ' (no status)'}: max rel err {err.max():.3e} at trajectory {worst}")
    assert err.max() < TOL, f"n {n}: max rel err {err.max():.3e} at trajectory {worst}"
    return float(err.max())


@pytest.mark.parametrize("r,M", TI.TWISTED, ids=_ids(TI.TWISTED))
@pytest.mark.parametrize("variant", TI.TILES, ids=[f"tile{t}" for t in TI.TILES])
@pytest.mark.parametrize("batch", ["guarded", "shifted", "looping"])
def test_general_kernel_against_the_oracle(gpu_ctx, exact, batch, variant, r, M):
    """guarded: n = tile - 1, the only tile is the guarded one.  shifted: n = tile + 1, one whole tile and the shifted last tile; once
    more without a status array.  looping: n = (4 CUs + 1) tile + 1, more tiles than waves -- a wave makes a second trip through the tile
    loop (prefetch, second input buffer, the aliased staging of the ALIAS instances) and the last tile is shifted."""
    tile, ref = variant, exact(r, M)
    if batch == "guarded":
        n = tile - 1
        _check_batch(gpu_ctx, ref, r, M, variant, n, 0, n - 1)
        if n == 3:
            _check_batch(gpu_ctx, ref, r, M, variant, n, 0, 1)
    elif batch == "shifted":
        n = tile + 1
        _check_batch(gpu_ctx, ref, r, M, variant, n, 1, n - 1)         # trajectory 1 belongs to both tiles
        _check_batch(gpu_ctx, ref, r, M, variant, n, 1, n - 1, status=False)
    else:
        n = (4 * _cus() + 1) * tile + 1
        _check_batch(gpu_ctx, ref, r, M, variant, n, 1, n - 1)


@pytest.mark.parametrize("r,M", TI.TWISTED, ids=_ids(TI.TWISTED))
@pytest.mark.parametrize("variant", TI.ONE_TILES, ids=[f"tile{t}" for t in TI.ONE_TILES])
def test_one_tile_kernel_against_the_oracle_and_bitwise_against_the_general_one(gpu_ctx, exact, variant, r, M):
    ref = exact(r, M)
    for n in (variant, 3 * variant):
        wp, T, bc = _inputs(r, M, n + 1)
        one, st = _solve(gpu_ctx, r, M, variant, wp[:n], T[:n], bc[:n])                    # one whole tile per wave
        assert np.all(st == UAVQP_SOLVED) and not _written(one)[1].any()
        err = _rel_err(one, ref[np.arange(n) % BASE])
        print(f"one tile {variant} r {r} M {M} n {n}: max rel err {err.max():.3e}")
        assert err.max() < TOL, f"n {n}: max rel err {err.max():.3e}"
        general, st = _solve(gpu_ctx, r, M, variant, wp, T, bc)                            # shifted last tile
        assert np.all(st == UAVQP_SOLVED)
        assert np.array_equal(_bits(one), _bits(general[:n])), (n, "coefficients of the leading trajectories differ between the paths")


@pytest.fixture
def fused(monkeypatch):
    monkeypatch.setenv("UAVQP_CAPTURE_LANE_NODES", "1")     # small captures are rebuilt
    monkeypatch.setenv("UAVQP_CAPTURE_LANES", "1")
    monkeypatch.setenv("UAVQP_CAPTURE_FUSE", "8")


@pytest.fixture(scope="module")
def ctx8():
    """A context of its own whose uniform solves launch at tile 8."""
    import uav_motion_planning_amd as U
    with U.Context(0) as ctx:
        ctx.set_variant(8)
        yield ctx


SOLVES, SETS = 6, 3      # one rotation: every buffer set is solved twice; with one lane a launch carries each set once


def _against_oracle(oracle, what, r, M, n, eager, inputs, bad_of):
    """Every valid trajectory of every buffer set of a rotation against the exact minimiser."""
    so = (np.arange(n + 1) * M).astype(np.int32)
    for s in range(SETS):
        wp, T, bc = inputs(s)
        bad = bad_of(s)
        valid = np.array([t for t in range(n) if t not in bad])
        Tv = np.array(T, dtype=np.float64).reshape(n, M)
        Tv[bad] = 1.0                                          # (the oracle is not asked about the invalid trajectories)
        ref, st = oracle.solve_exact_batch(r, so, np.asarray(wp).reshape(n, M + 1, 3), Tv, np.asarray(bc).reshape(n, 2, r - 1, 3))
        assert np.all(st == 0)
        got = eager[f"out{s}"].cpu().numpy().reshape(n, -1)[valid]
        err = _rel_err(got, ref.reshape(n, -1)[valid])
        print(f"{what} r {r} M {M} n {n} set {s}: max rel err {err.max():.3e}")
        assert err.max() < TOL, f"set {s}: max rel err {err.max():.3e}"


def _tile4(ctx, rules, oracle, what, r, M, n):
    report = {}
    eager = G._rotation(ctx, rules, r, M, n, 1, 8, SOLVES, SETS, has_group=(r, M) in TI.GROUP[4], has_group8=(r, M) in TI.GROUP8, report=report)
    bad = [t for t, _ in G._bad(n, M)]
    _against_oracle(oracle, what, r, M, n, eager, lambda s: G._host_inputs(r, M, n, 900 + s, tuple(G._bad(n, M)) if s == 0 else ()),
                    lambda s: bad if s == 0 else [])
    return report["launches"], report["kernels"]


def _tile8(ctx, rules, oracle, what, r, M, n):
    plan, choose = rules
    eager, launches = F._rotation(ctx, plan, r, M, n, 8, 1, 8, SOLVES, SETS, has_group=(r, M) in TI.GROUP[8])
    _against_oracle(oracle, what, r, M, n, eager, lambda s: O._inputs(r, M, n, seed=500 + s, bad=F.BAD if s == 0 else None),
                    lambda s: [F.BAD[0]] if s == 0 else [])
    return launches, [choose(len(g), r, M, 8, n) for g in launches]


@pytest.mark.parametrize("r,M", TI.GROUP[4], ids=_ids(TI.GROUP[4]))
def test_group_kernel_at_tile_4(gpu_ctx, host_rules, oracle, fused, r, M):
    """n = 12, no whole number of eights: three waves of the 16-lane group kernel per member."""
    launches, kernels = _tile4(gpu_ctx, host_rules, oracle, "group tile 4", r, M, 12)
    assert sorted(len(g) for g in launches) == [SETS, SETS] and kernels == [G.OWN_TILE, G.OWN_TILE]


@pytest.mark.parametrize("r,M", TI.GROUP8, ids=_ids(TI.GROUP8))
def test_group8_kernel(gpu_ctx, host_rules, oracle, fused, r, M):
    """n = 24 at tile 4: three waves of eight trajectories per member."""
    launches, kernels = _tile4(gpu_ctx, host_rules, oracle, "group8", r, M, 24)
    assert sorted(len(g) for g in launches) == [SETS, SETS] and kernels == [G.EIGHT_PER_WAVE, G.EIGHT_PER_WAVE]


@pytest.mark.parametrize("r,M", TI.GROUP[8], ids=_ids(TI.GROUP[8]))
def test_group_kernel_at_tile_8(ctx8, host_rules, oracle, fused, r, M):
    """n = 24 at tile 8: three waves of the 8-lane group kernel per member."""
    launches, kernels = _tile8(ctx8, host_rules, oracle, "group tile 8", r, M, 24)
    assert sorted(len(g) for g in launches) == [SETS, SETS] and kernels == [G.OWN_TILE, G.OWN_TILE]


@pytest.mark.parametrize("r,M", NO_GROUP[4], ids=_ids(NO_GROUP[4]))
def test_shapes_without_a_group_kernel_at_tile_4_replay_one_launch_per_solve(gpu_ctx, host_rules, oracle, fused, r, M):
    for n in (12, 24):
        launches, kernels = _tile4(gpu_ctx, host_rules, oracle, "unfused tile 4", r, M, n)
        assert [len(g) for g in launches] == [1] * SOLVES and kernels == [G.AS_CAPTURED] * SOLVES


@pytest.mark.parametrize("r,M", NO_GROUP[8], ids=_ids(NO_GROUP[8]))
def test_shapes_without_a_group_kernel_at_tile_8_replay_one_launch_per_solve(ctx8, host_rules, oracle, fused, r, M):
    launches, kernels = _tile8(ctx8, host_rules, oracle, "unfused tile 8", r, M, 24)
    assert [len(g) for g in launches] == [1] * SOLVES and kernels == [G.AS_CAPTURED] * SOLVES
