"""GPU: the latency shapes of the register-resident solve (tile 4 = 16 lanes per trajectory, tile 8 = 8 lanes) have two instantiations.
A launch of exactly one WHOLE tile per wave (n_traj a multiple of the tile, no more tiles than 4 waves per CU) takes the one without
the shifted / guarded tile, the prefetch and the second input buffer; every other batch takes the general one.  Neighbouring batch sizes
therefore take the two paths and no switch is needed: n = k * TILE is the new path, n + 1 (shifted last tile) and n + TILE (one more
tile; for k = 4 * CUs the first batch whose waves loop) are the general one.  Nothing differs in the arithmetic, so the leading n
trajectories must agree BIT FOR BIT.  Oracle tolerance: that of tests/test_gpu_parity.py (1e-9 relative per trajectory, 'distance'
durations)."""
import numpy as np
import pytest

from uav_motion_planning_amd import UAVQP_INVALID_INPUT, UAVQP_SOLVED
from uav_motion_planning_amd import workloads as W

pytestmark = pytest.mark.gpu

SHAPES = [(4, 8), (4, 7), (4, 3), (3, 16), (3, 5), (3, 2)]     # odd M: halves of different length
VARIANTS = [4, 8]                                             # = the tile; 16 resp. 8 lanes per trajectory
BASE = 97                                                     # distinct trajectories; larger batches repeat them (odd: tiles differ)
SENTINEL = 12345.678
_cache = {}


def _base(r, M):
    if (r, M) not in _cache:
        b = W.uniform_batch(300 + 10 * r + M, BASE, M, r, time_mode="distance")
        b["bc"] = np.random.default_rng(7 * r + M).uniform(-2.0, 2.0, size=b["bc"].shape)    # every boundary derivative non-zero
        _cache[(r, M)] = b
    return _cache[(r, M)]


def _inputs(r, M, n):
    b = _base(r, M)
    idx = np.arange(n) % BASE
    return b["waypoints"][idx].copy(), b["times"][idx].copy(), b["bc"][idx].copy()


def _solve(ctx, r, M, variant, wp, T, bc, status=True, misalign=False):
    """Device entry on fresh tensors; the coefficient rows are pre-filled with SENTINEL, the statuses with -77."""
    import torch
    dev = torch.device("cuda", 0)
    n = T.shape[0]

    def put(a):
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        t = torch.empty(a.size + 1, dtype=torch.float64, device=dev)
        v = t[1:] if misalign else t[:-1]        # misalign: the view starts 8 bytes into a 256-byte aligned allocation
        v.copy_(torch.from_numpy(a))
        return v

    d_wp, d_T, d_bc = put(wp), put(T), put(bc)
    d_c = put(np.full(n * 3 * M * 2 * r, SENTINEL))
    d_st = torch.full((n,), -77, dtype=torch.int32, device=dev) if status else None
    torch.cuda.synchronize()                     # the fills above ran on torch's stream, the solve runs on the ctx's
    ctx.set_variant(variant)
    try:
        ctx.solve_batch_device(r, n, M, M, None, d_wp, d_T, d_bc, d_c, d_st)
        ctx.synchronize()
    finally:
        ctx.set_variant(0)
    torch.cuda.synchronize()
    return d_c.cpu().numpy().reshape(n, -1), (d_st.cpu().numpy() if status else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _rel_err(got, ref):
    return np.max(np.abs(got - ref), axis=1) / np.maximum(np.max(np.abs(ref), axis=1), 1e-300)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("r,M", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_prefix_is_bitwise_equal_across_the_two_paths(gpu_ctx, variant, r, M):
    tile = variant
    for k in (1, 3, 4 * _cus()):
        n = k * tile
        wp, T, bc = _inputs(r, M, n + tile)
        c0, s0 = _solve(gpu_ctx, r, M, variant, wp[:n], T[:n], bc[:n])              # one whole tile per wave
        assert np.all(s0 == UAVQP_SOLVED), (k, s0)
        for n2 in (n + 1, n + tile):                                                # shifted last tile; one more tile
            c1, s1 = _solve(gpu_ctx, r, M, variant, wp[:n2], T[:n2], bc[:n2])
            assert np.all(s1 == UAVQP_SOLVED), (k, n2)
            assert np.array_equal(_bits(c0), _bits(c1[:n])), (k, n2, "coefficients of the leading trajectories differ between the paths")


@pytest.fixture(scope="module")
def exact(oracle):
    """oracle.solve_exact_batch of the first 3 * 8 base trajectories of a shape, computed once and shared."""
    memo = {}

    def get(r, M):
        if (r, M) not in memo:
            n = 24
            wp, T, bc = _inputs(r, M, n)
            so = (np.arange(n + 1) * M).astype(np.int32)
            ref, st = oracle.solve_exact_batch(r, so, wp, T, bc)
            assert np.all(st == 0)
            ref = ref.reshape(n, -1)
            ref.setflags(write=False)
            memo[(r, M)] = ref
        return memo[(r, M)]
    return get


@pytest.mark.parametrize("r,M", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_one_tile_path_agrees_with_the_oracle(gpu_ctx, exact, variant, r, M):
    ref = exact(r, M)
    for n in (variant, 3 * variant):
        wp, T, bc = _inputs(r, M, n)
        got, st = _solve(gpu_ctx, r, M, variant, wp, T, bc)
        err = _rel_err(got, ref[:n])
        print(f"variant {variant} r {r} M {M} n {n}: max rel err {err.max():.3e}")
        assert np.all(st == UAVQP_SOLVED)
        assert err.max() < 1e-9, f"max rel err {err.max():.3e}"


@pytest.mark.parametrize("r,M", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_edge_batches_stay_on_the_general_path_and_stay_correct(gpu_ctx, exact, variant, r, M):
    ref = exact(r, M)
    n = variant - 1                                        # smaller than a tile: the guarded loads
    wp, T, bc = _inputs(r, M, n)
    got, st = _solve(gpu_ctx, r, M, variant, wp, T, bc)
    assert np.all(st == UAVQP_SOLVED) and _rel_err(got, ref[:n]).max() < 1e-9
    n = 3 * variant                                        # whole tiles, but no array 16-byte aligned: the generic kernel
    wp, T, bc = _inputs(r, M, n)
    got, st = _solve(gpu_ctx, r, M, 0, wp, T, bc, misalign=True)
    assert np.all(st == UAVQP_SOLVED) and _rel_err(got, ref[:n]).max() < 1e-9


@pytest.mark.parametrize("r,M", [(4, 8), (4, 7), (3, 5)])
@pytest.mark.parametrize("variant", VARIANTS)
def test_invalid_durations_on_the_one_tile_path(gpu_ctx, variant, r, M):
    tile, n = variant, 3 * variant
    wp, T, bc = _inputs(r, M, n)
    clean, st = _solve(gpu_ctx, r, M, variant, wp, T, bc)
    assert np.all(st == UAVQP_SOLVED)
    first, last = tile, 2 * tile - 1                       # first and last trajectory of the middle tile
    seg_L, seg_R = 0, M - 1                                # a segment of the forward half, one of the reversed half
    for bad in (0.0, -1.0, np.inf, np.nan):
        for seg_first, seg_last in ((seg_L, seg_R), (seg_R, seg_L)):
            Tb = T.copy()
            Tb[first, seg_first] = bad
            Tb[last, seg_last] = bad
            got, st = _solve(gpu_ctx, r, M, variant, wp, Tb, bc)
            assert list(st[[first, last]]) == [UAVQP_INVALID_INPUT] * 2, (bad, st)
            assert np.all(got[[first, last]] == SENTINEL), (bad, "coefficient rows of an invalid trajectory were written")
            others = np.delete(np.arange(n), [first, last])
            assert np.all(st[others] == UAVQP_SOLVED)
            assert np.array_equal(_bits(got[others]), _bits(clean[others])), (bad, "a neighbour of an invalid trajectory changed")


@pytest.mark.parametrize("variant", VARIANTS)
def test_null_status_on_the_one_tile_path(gpu_ctx, variant):
    r, M, n = 4, 8, 3 * variant
    wp, T, bc = _inputs(r, M, n)
    with_st, st = _solve(gpu_ctx, r, M, variant, wp, T, bc)
    without, none = _solve(gpu_ctx, r, M, variant, wp, T, bc, status=False)
    assert none is None and np.all(st == UAVQP_SOLVED)
    assert np.array_equal(_bits(with_st), _bits(without))
