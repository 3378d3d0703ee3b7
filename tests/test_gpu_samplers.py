"""-m gpu: the four samplers of include/uavqp.h -- uavqp_eval_batch_device (eval_kernel), uavqp_traj_length_device (traj_length_kernel),
uavqp_ellipsoid_check_device (ellipsoid_kernel), uavqp_ellipsoid_check_grid_device (ellipsoid_grid_kernel) -- against the restatement of
the header in tests/sampler_reference.py: the segment rule in float64 exactly as stated, everything else in np.longdouble.

Inputs are designed, not solved: all coefficients distinct, neighbouring segments discontinuous in value and every derivative, time
grids exact by construction (tests/test_sampler_contract.py checks all of that on the CPU, and that nothing has to be skipped).
Tolerances: evaluation 32 * 2^-53 * S per value, S = sum_j f_j |c_j| |t|^(j-d) (Horner with one rounding per step over at most 8
coefficients plus the factor product is bounded by about 18 * 2^-53 * S); length: that bound on both ends of every chord, summed, plus
n * 2^-53 * length for the parallel sum; sample counts, verdicts and first_hit are exact.  Largest device error measured on an
MI355X: docs/measurement_log.md."""
import ctypes

import numpy as np
import pytest

import sampler_reference as R
import uav_motion_planning_amd as U
from uav_motion_planning_amd import _lib

pytestmark = pytest.mark.gpu
LD = R.LD
TOL = LD(32 * R.U53)
INVALID = _lib.UAVQP_ERR_INVALID_ARG


def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _batch(case, first=0, count=None):
    """Device copies of trajectories first .. first + count of a case: (n, uniform, d_so or None, d_T, d_c, host so of the slice)."""
    count = case["n_traj"] - first if count is None else count
    so = case["seg_offsets64"]
    s0, s1 = int(so[first]), int(so[first + count])
    nc = 2 * case["r"]
    sub = (so[first:first + count + 1] - s0)
    T, c = case["times"][s0:s1], case["coeff"][3 * nc * s0:3 * nc * s1]
    d_so = None if case["uniform"] > 0 else _up(sub.astype(np.int32))
    return count, case["uniform"], d_so, _up(T if T.size else np.zeros(1)), _up(c if c.size else np.zeros(1)), sub


# ---------------------------------------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------------------------------------
def _eval(ctx, r, batch, n_samples, t0, dt, what, misalign=False):
    """NaN-filled output with one guard double on each side; with misalign the output starts 8 bytes into the allocation."""
    import torch
    n, uni, d_so, d_T, d_c, _ = batch
    K = bin(what & 7).count("1")
    size = n * n_samples * K * 3
    lead = 1 if misalign else 2                                             # torch allocations are 256-byte aligned: +8 is not 16-byte aligned
    buf = torch.full((lead + size + 1,), float("nan"), dtype=torch.float64, device=_dev())
    out = buf[lead:lead + size]
    assert (out.data_ptr() % 16 == 8) == misalign
    ctx.eval_batch_device(r, n, uni, d_so, d_T, d_c, n_samples, t0, dt, what, out)
    ctx.synchronize()
    h = buf.cpu().numpy()
    assert np.isnan(h[:lead]).all() and np.isnan(h[-1]), "wrote outside its output"
    return h[lead:lead + size].reshape(n, n_samples, K, 3)


def _check_eval(tag, got, ref, what, first=0, count=None, n_samples=None, worst=None):
    count = got.shape[0] if count is None else count
    n_samples = got.shape[1] if n_samples is None else n_samples
    want = R.select_what(ref["out"][first:first + count, :n_samples], what)
    S = R.select_what(ref["S"][first:first + count, :n_samples], what)
    assert np.isfinite(got).all(), tag                                      # every element written
    err = np.abs(LD(1) * got - want)
    zero = ref["M"][first:first + count] == 0
    assert not got[zero].any(), tag                                         # zero-segment trajectory: rows of zeros
    ratio = float(np.max(np.where(S > 0, err / np.where(S > 0, TOL * S, 1), np.where(err > 0, np.inf, 0))))
    if worst is not None:
        worst.append(ratio)
    bad = np.argwhere(err > TOL * S)
    assert bad.size == 0, (tag, ratio, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", ["uniform17", "ragged"])
@pytest.mark.parametrize("r", [3, 4])
def test_eval_every_designed_sample_and_mask(gpu_ctx, r, name):
    case = R.eval_cases(r)[name]
    batch = _batch(case)
    worst = []
    for g in case["grids"]:
        for what in range(1, 8):
            for mis in ((False, True) if g["kind"] in ("window", "coarse") else (False,)):
                got = _eval(gpu_ctx, r, batch, g["n_samples"], g["t0"], g["dt"], what, misalign=mis)
                _check_eval(f"r{r}-{name}-{g['name']}-what{what}-mis{mis}", got, g["ref"], what, worst=worst)
    print(f"r{r}-{name}: largest error {max(worst):.3f} of the bound 32 * 2^-53 * S")


@pytest.mark.parametrize("n,n_samples", [(1, 1), (5, 51), (3, 85), (4, 64), (1, 257)])
def test_eval_small_totals_and_odd_tails(gpu_ctx, n, n_samples):
    """1, 255, 255, 256 and 257 samples in all; an odd total with K = 1 and K = 3 leaves an odd number of doubles in the tail block.
    The first n trajectories of the uniform batch on the first n_samples samples of its coarse grid, aligned and not."""
    for r in (3, 4):
        case = R.eval_cases(r)["uniform17"]
        g = next(x for x in case["grids"] if x["kind"] == "coarse")
        batch = _batch(case, 0, n)
        for what in (1, 2, 4, 7, 5):
            for mis in (False, True):
                got = _eval(gpu_ctx, r, batch, n_samples, g["t0"], g["dt"], what, misalign=mis)
                _check_eval(f"r{r}-{n}x{n_samples}-what{what}-mis{mis}", got, g["ref"], what, 0, n, n_samples)


def test_eval_beyond_one_grid_of_blocks(gpu_ctx):
    """The launch is capped at 16 * multi_processor_count blocks of 256 samples and then strides: three trajectories with just more
    samples than that in all, what = 1, compared in full."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    r = 3
    case = R.eval_cases(r)["uniform17"]
    n = 3
    n_samples = (256 * 16 * cus) // n + 77
    assert n * n_samples > 256 * 16 * cus
    t0, dt = -0.125, 2.0 ** -14
    ref = R.eval_reference(r, n, 17, None, case["times"][:17 * n], case["coeff"][:3 * 6 * 17 * n], n_samples, t0, dt)
    assert ref["exact"].all() and ref["clamped"][:, -1].all() and not ref["clamped"][:, n_samples // 3].any()
    got = _eval(gpu_ctx, r, _batch(case, 0, n), n_samples, t0, dt, 1)
    _check_eval("beyond one grid", got, ref, 1)


def test_eval_arguments(gpu_ctx):
    import torch
    lib = U.lib()
    case = R.eval_cases(3)["ragged"]
    n, uni, d_so, d_T, d_c, _ = _batch(case)
    out = torch.full((n * 4 * 9,), float("nan"), dtype=torch.float64, device=_dev())

    def call(r=3, n=n, uni=0, so=d_so, T=d_T, c=d_c, ns=4, what=7, o=out):
        rc = lib.uavqp_eval_batch_device(gpu_ctx._h, r, n, uni, _p(so), _p(T), _p(c), ns, 0.0, 0.25, what, _p(o))
        gpu_ctx.synchronize()
        return rc

    for bad in (dict(what=0), dict(what=8), dict(r=5), dict(r=2), dict(n=-1), dict(ns=-1), dict(uni=-1), dict(T=None), dict(c=None), dict(o=None),
                dict(so=None)):
        assert call(**bad) == INVALID, bad
        assert bool(torch.isnan(out).all()), bad
    assert call(ns=0) == _lib.UAVQP_OK and call(n=0) == _lib.UAVQP_OK and bool(torch.isnan(out).all())        # n_samples == 0 writes nothing
    assert call(what=15) == _lib.UAVQP_OK and not bool(torch.isnan(out).any())                                # only the low three bits count


# ---------------------------------------------------------------------------------------------------------------------------------
# length
# ---------------------------------------------------------------------------------------------------------------------------------
def _length(ctx, case, want=(True, True, True), dt=None):
    import torch
    n, uni, d_so, d_T, d_c, _ = _batch(case)
    L = torch.full((n,), -7.0, dtype=torch.float64, device=_dev()) if want[0] else None
    V = torch.full((n,), -7.0, dtype=torch.float64, device=_dev()) if want[1] else None
    N = torch.full((n,), -7, dtype=torch.int32, device=_dev()) if want[2] else None
    ctx.traj_length_device(case["r"], n, uni, d_so, d_T, d_c, dt=case["dt"] if dt is None else dt, length=L, mean_vel=V, n_samples=N)
    ctx.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in (L, V, N))


@pytest.mark.parametrize("name", ["dyadic", "line", "accumulated", "slack", "threshold"])
@pytest.mark.parametrize("r", [3, 4])
def test_length_count_and_mean_velocity(gpu_ctx, r, name):
    case = R.length_cases(r)[name]
    ref = case["ref"]
    L, V, N = _length(gpu_ctx, case)
    assert np.array_equal(N, ref["n"]), (N, ref["n"])                       # the accumulated count, exactly
    errL = np.abs(LD(1) * L - ref["length"])
    live = ref["length"] > 0
    print(f"r{r}-{name}: length error at most {float(np.max(errL[live] / ref['bound'][live])):.3f} of the derived bound")
    assert np.all(errL <= ref["bound"]), (errL, ref["bound"])
    assert np.all(L[~live] == 0)
    zero = ref["total"] == 0
    assert np.isnan(V[zero]).all() and np.array_equal(N[zero], np.zeros(int(zero.sum()), dtype=np.int32))     # zero segments: 0 samples, length 0, mean 0 / 0
    tot = LD(1) * ref["total"][~zero]
    assert np.all(np.abs(LD(1) * V[~zero] - ref["mean"][~zero]) <= ref["bound"][~zero] / tot + LD(2 * R.U53) * ref["mean"][~zero])
    assert np.array_equal(V[~zero], L[~zero] / ref["total"][~zero])         # mean velocity IS length / total time
    # outputs NULL one at a time: the others are the same bytes
    for k in range(3):
        want = [True] * 3
        want[k] = False
        part = _length(gpu_ctx, case, want=tuple(want))
        for j, full in enumerate((L, V, N)):
            assert part[j] is None if j == k else part[j].tobytes() == full.tobytes()


def test_length_arguments(gpu_ctx):
    import torch
    lib = U.lib()
    case = R.length_cases(3)["dyadic"]
    n, uni, d_so, d_T, d_c, _ = _batch(case)
    L = torch.full((n,), -7.0, dtype=torch.float64, device=_dev())

    def call(r=3, n=n, uni=0, so=d_so, T=d_T, c=d_c, dt=R.LENGTH_DT):
        rc = lib.uavqp_traj_length_device(gpu_ctx._h, r, n, uni, _p(so), _p(T), _p(c), dt, _p(L), None, None)
        gpu_ctx.synchronize()
        return rc

    for bad in (dict(dt=0.0), dict(dt=-0.01), dict(dt=float("nan")), dict(dt=float("inf")), dict(r=5), dict(n=-1), dict(uni=-1), dict(T=None),
                dict(c=None), dict(so=None)):
        assert call(**bad) == INVALID, bad
        assert bool((L == -7.0).all()), bad
    assert call(n=0) == _lib.UAVQP_OK and bool((L == -7.0).all())
    assert call() == _lib.UAVQP_OK and not bool((L == -7.0).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# ellipsoid check: exhaustive and grid
# ---------------------------------------------------------------------------------------------------------------------------------
CELLS = (R.RAD, 1.0, 0.25)              # equal to the search radius (27 cells), coarser, finer (the kernel's other branch)


def _check_both(ctx, case, with_flags=True, cells=CELLS):
    """Exhaustive entry and grid entry (every cell size) on one case.  Returns [(tag, first_hit, flags or None), ...]."""
    import torch
    n, uni, d_so, d_T, d_c, _ = _batch(case)
    r, ns = case["r"], case["n_samples"]
    obs = case["obs"]
    d_obs = _up(obs)
    out = []

    def fresh():
        fh = torch.full((n,), -5, dtype=torch.int32, device=_dev())
        fl = torch.full((n * ns + 1,), 9, dtype=torch.uint8, device=_dev()) if with_flags else None
        return fh, fl

    def done(tag, fh, fl):
        ctx.synchronize()
        if fl is not None:
            h = fl.cpu().numpy()
            assert h[-1] == 9, tag
            out.append((tag, fh.cpu().numpy(), h[:-1].reshape(n, ns)))
        else:
            out.append((tag, fh.cpu().numpy(), None))

    fh, fl = fresh()
    ctx.ellipsoid_check_device(r, n, uni, d_so, d_T, d_c, ns, case["t0"], case["dt"], d_obs, obs.shape[0], R.ROBOT_R, R.ROBOT_H, fh, fl)
    done("exhaustive", fh, fl)
    for cell in cells:
        grid = ctx.obstacle_grid_build(d_obs, obs.shape[0], cell)
        try:
            fh, fl = fresh()
            ctx.ellipsoid_check_grid_device(r, n, uni, d_so, d_T, d_c, ns, case["t0"], case["dt"], grid, R.ROBOT_R, R.ROBOT_H, fh, fl)
            done(f"grid cell {cell}", fh, fl)
        finally:
            ctx.obstacle_grid_destroy(grid)
    return out


def _assert_verdicts(name, case, results):
    ref = case["ref"]
    for tag, fh, fl in results:
        assert np.array_equal(fh, ref["first_hit"]), (name, tag, fh, ref["first_hit"])
        if fl is not None:
            bad = np.argwhere(fl != ref["flags"])
            assert bad.size == 0, (name, tag, bad[:6])
            assert fl.tobytes() == results[0][2].tobytes()                  # bit-identical to the exhaustive entry


def _ell_case(r, name):
    if name == "endpoint":
        return R.endpoint_case(r)
    if name in R.knot_cases(r):
        return R.knot_cases(r)[name]
    if name == "endpoint_lane0":
        return R.endpoint_lane0_case(r)
    if name == "degenerate":
        return R.degenerate_case(r)
    if name in R.grid_geometry_cases(r):
        return R.grid_geometry_cases(r)[name]
    return R.ellipsoid_cases(r)[name]


ELL_NAMES = ["directions", "tile1", "tile1024", "tile1025", "ragged", "blocks", "endpoint", "endpoint_lane0", "knot_window", "knot_threshold", "knot_above", "degenerate", "neighbours", "bbox", "pooled", "pooled_miss"]


@pytest.mark.parametrize("name", ELL_NAMES)
@pytest.mark.parametrize("r", [3, 4])
def test_ellipsoid_verdicts_exhaustive_and_grid(gpu_ctx, r, name):
    """Flags and first_hit of both entry points are the reference's, exactly, with flags and with flags = NULL (the grid kernel then
    leaves out repeated past-the-end samples: first_hit must not change)."""
    case = _ell_case(r, name)
    _assert_verdicts(name, case, _check_both(gpu_ctx, case, with_flags=True))
    _assert_verdicts(name, case, _check_both(gpu_ctx, case, with_flags=False))


def test_ellipsoid_beyond_one_grid_of_blocks(gpu_ctx):
    """More samples than one launch holds (16 * CUs blocks of 256; the grid entry: 64 * CUs waves), an 8-point cloud.  Two short
    trajectories: the first collides at its end point -- every past-the-end sample is a hit, also in the strided rounds, and first_hit
    stays the first of them --, the second at one interior sample only."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = R.beyond_grid_case(3, cus)
    ns, ref = case["n_samples"], case["ref"]
    assert 2 * ns > 256 * 16 * cus and 2 * ns > 64 * 64 * cus and ref["exact"].all()
    assert ref["first_hit"][1] == 5 and 0 < ref["first_hit"][0] < 20 and ref["flags"][0].sum() == ns - ref["first_hit"][0]
    _assert_verdicts("beyond one grid", case, _check_both(gpu_ctx, case, with_flags=True, cells=(R.RAD,)))
    _assert_verdicts("beyond one grid", case, _check_both(gpu_ctx, case, with_flags=False, cells=(R.RAD,)))
