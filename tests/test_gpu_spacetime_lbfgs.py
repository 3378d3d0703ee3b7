"""-m gpu: the joint waypoint / duration optimiser with limited-memory BFGS directions (uavqp_spacetime_lbfgs_device / _host) against the
designed reference of tests/spacetime_reference.py (the oracle's exact solve, the longdouble penalties, the recorded optima of scipy's
L-BFGS-B in tests/golden/spacetime_scipy.json) and against the projected-gradient entry uavqp_spacetime_optimize_device.

Scene, cases, limits, seeds and the device harness are those of tests/test_gpu_spacetime.py (imported, not copied): 32 x 32 x 16 voxels of
0.25 m; the ragged batch of 14 trajectories plus the designed invalid one, the uniform batch of 8 x 4 segments, and 4 x 11 segments; r = 3
and 4; max_move = 1 m.

Bounds.  Objective at the start and at the returned point against the reference's f there: 1e-9 relative; min_dist: 1e-9 x max(|reference|,
one voxel); peaks 1e-9 relative (the bounds of tests/test_gpu_spacetime.py).  Against scipy: gap = (f_lib - f_scipy) / (f_start - f_scipy)
<= min(4 x Q.GAP_LBFGS_AT_DEFAULT, R.GAP_AT_DEFAULT / 2) at the default 32 trials.  Factor 4: on the CPU, perturbations far larger than
rounding (memory 8 -> 4, max_backtracks 6 -> 3: tools/spacetime_convergence.py --method lbfgs) moved the transcription's worst gap by up to
2.3 x; doubling that leaves room for another floating-point order.  The second term keeps the test from passing with something no better
than gradient descent.  Feasibility: the three comparisons of tests/test_gpu_spacetime.py at Q.FEASIBILITY_ITERS = 64 trials for all three
runs (the transcription meets them at 64 on all 44 trajectories: the same tool).  Everything else is exact.

Measured on MI355X: docs/measurement_log.md, "Joint optimiser with limited-memory BFGS directions"."""
import ctypes
import json
import math

import numpy as np
import pytest

import uav_motion_planning_amd as U
from uav_motion_planning_amd import _lib
from uav_motion_planning_amd.esdf import EsdfMap

import spacetime_lbfgs_reference as Q
import spacetime_reference as R
import test_gpu_spacetime as G
import waypoint_opt_reference as W

pytestmark = pytest.mark.gpu
MOVE = G.MOVE
GAP_BOUND = min(4.0 * Q.GAP_LBFGS_AT_DEFAULT, R.GAP_AT_DEFAULT / 2.0)
OUT_KEYS = G.OUT_KEYS
KINDS, IDS, SCIPY_KINDS, SCIPY_IDS = G.KINDS, G.IDS, G.SCIPY_KINDS, G.SCIPY_IDS
valid_ids, original_index = G.valid_ids, G.original_index


def defaults():
    p = _lib.SpacetimeLbfgsParams()
    _lib.lib().uavqp_default_spacetime_lbfgs_params(ctypes.byref(p))
    return p


@pytest.fixture(scope="module")
def esdf(gpu_ctx):
    sc = R.scene()
    m = EsdfMap(gpu_ctx, W.DIMS, W.ORIGIN, W.RES, W.MAX_DIST)
    m.set_occupancy(sc["occ"])
    m.update()
    gpu_ctx.synchronize()
    yield m
    m.close()


class Dev(G.Dev):
    """The harness of tests/test_gpu_spacetime.py with the new entry beside the old one (optimize: uavqp_spacetime_optimize_device)."""

    def lbfgs(self, esdf, wp=None, T=None, limits=None, clearance=None, total=None, so=True, null=(), **params):
        t = self.torch
        d_wp, d_T = self.up(self.wp0 if wp is None else wp), self.up(self.T0 if T is None else T)
        out = dict(coeff=self.zeros(3 * 2 * self.r * self.total), status=self.zeros(self.n, t.int32), obj=self.zeros((self.n, 2)),
                   acc=self.zeros(self.n, t.int32), peak=self.zeros((self.n, 2)), md=self.zeros(self.n), outside=self.zeros(self.n, t.int32))
        params.setdefault("max_move", MOVE)
        arg = {k: (None if k in null else v) for k, v in out.items()}
        t.cuda.synchronize()
        self.ctx.spacetime_lbfgs_device(self.r, self.n, self.uni, self.mmax, self.total if total is None else total,
                                        self.d_so if so else None, d_wp, d_T, self.d_bc, esdf, arg["coeff"], arg["status"], arg["obj"],
                                        arg["acc"], arg["peak"], arg["md"], arg["outside"], limits=dict(R.LIMITS_OF[self.r], **(limits or {})),
                                        clearance=dict(R.CLEARANCE, **(clearance or {})), **params)
        self.ctx.synchronize()
        res = {k: v.cpu().numpy() for k, v in out.items()}
        res["wp"], res["T"] = d_wp.cpu().numpy(), d_T.cpu().numpy()
        res["d_wp"], res["d_T"] = d_wp, d_T
        res["bc"] = self.d_bc.cpu().numpy()
        return res


def make(gpu_ctx, r, kind):
    """-> (Dev, index of the invalid trajectory or None)"""
    if kind == "ragged":
        b, bad = G.with_invalid(R.cases(r))
        return Dev(gpu_ctx, b, False), bad
    return Dev(gpu_ctx, R.batch_of(r, kind), True), None


_runs = {}


def run_of(gpu_ctx, esdf, r, kind):
    """The default-parameter run of one of the three batches (computed once per module): (Dev, result, index of the invalid trajectory)."""
    key = (r, kind)
    if key not in _runs:
        d, bad = make(gpu_ctx, r, kind)
        _runs[key] = (d, d.lbfgs(esdf), bad)
    return _runs[key]


def check_invariants(d, res, bad, esdf, max_iters, t_min, t_max, every_valid_moves=True):
    ok = valid_ids(d, bad)
    st = res["status"]
    assert np.all(st[ok] == U.UAVQP_SOLVED)
    assert np.all(res["obj"][ok, 1] <= res["obj"][ok, 0])
    assert np.all(res["acc"] >= 0) and np.all(res["acc"] <= max_iters)
    assert np.array_equal(res["bc"], d.bc0)
    lo, hi = d.wp0 - MOVE, d.wp0 + MOVE
    assert np.all(res["wp"] >= lo) and np.all(res["wp"] <= hi)
    seg_ok = d.seg_traj != (-1 if bad is None else bad)
    assert np.all(res["T"][seg_ok] >= t_min) and np.all(res["T"][seg_ok] <= t_max)
    for t in range(d.n):
        k0, k1 = int(d.so[t]) + t, int(d.so[t + 1]) + t
        s0, s1 = int(d.so[t]), int(d.so[t + 1])
        assert res["wp"][[k0, k1]].tobytes() == d.wp0[[k0, k1]].tobytes(), "an end knot moved"
        if t == bad:
            assert st[t] == U.UAVQP_INVALID_INPUT
            assert res["wp"][k0:k1 + 1].tobytes() == d.wp0[k0:k1 + 1].tobytes() and res["T"][s0:s1].tobytes() == d.T0[s0:s1].tobytes()
            assert np.all(np.isnan(res["obj"][t])) and res["acc"][t] == 0
        elif every_valid_moves:
            assert res["acc"][t] > 0 and res["obj"][t, 1] < res["obj"][t, 0], f"trajectory {t} was left out"
            assert np.any(res["T"][s0:s1] != d.T0[s0:s1])
            if s1 - s0 == 1:
                assert res["wp"][k0:k1 + 1].tobytes() == d.wp0[k0:k1 + 1].tobytes(), "the M = 1 trajectory changes only its duration"
            else:
                assert np.any(res["wp"][k0:k1 + 1] != d.wp0[k0:k1 + 1])
    # the coefficients and the status are a plain solve at the point handed back
    fresh, st2 = d.solve(res["d_wp"], res["d_T"])
    assert fresh.cpu().numpy().tobytes() == res["coeff"].tobytes() and np.array_equal(st2.cpu().numpy(), st)
    # the diagnostics are the fused penalty's at the point handed back
    pen = d.flight(esdf, res["d_T"], fresh, st2, want=("peak", "min_dist", "outside"))
    assert pen["peak"].tobytes() == res["peak"].tobytes() and pen["min_dist"].tobytes() == res["md"].tobytes()
    assert np.array_equal(pen["outside"], res["outside"])


# ---------------------------------------------------------------------------------------------------
# invariants, all exact
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,kind", KINDS, ids=IDS)
def test_lbfgs_invariants(gpu_ctx, esdf, r, kind):
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    P = defaults()
    check_invariants(d, res, bad, esdf, P.max_iters, P.t_min, P.t_max)
    # run to run: identical bytes (NaN objectives of the invalid trajectory compared as bytes too)
    again = d.lbfgs(esdf)
    for k in OUT_KEYS:
        assert res[k].tobytes() == again[k].tobytes(), k
    ok = valid_ids(d, bad)
    print(f"r={r} {kind}: median f_result / f_start {np.median(res['obj'][ok, 1] / res['obj'][ok, 0]):.4f}, accepted min / median / max "
          f"{res['acc'][ok].min()} / {int(np.median(res['acc'][ok]))} / {res['acc'][ok].max()} of {P.max_iters}")


@pytest.mark.parametrize("r", [3, 4])
def test_lbfgs_uniform_call_equals_ragged_call(gpu_ctx, esdf, r):
    """Eleven segments: no specialised solve kernel, so both calls run the same solve and every byte must agree."""
    d, res, _ = run_of(gpu_ctx, esdf, r, "uniform11")
    other = Dev(gpu_ctx, d.b, False).lbfgs(esdf)
    for k in OUT_KEYS:
        assert res[k].tobytes() == other[k].tobytes(), k


@pytest.mark.parametrize("r,kind", [(3, "ragged"), (4, "uniform")], ids=["r3-ragged", "r4-uniform"])
def test_lbfgs_host_entry_equals_device_entry(gpu_ctx, esdf, r, kind):
    d, res, _ = run_of(gpu_ctx, esdf, r, kind)
    got = gpu_ctx.spacetime_lbfgs_host(r, d.so, d.wp0, d.T0, d.bc0, esdf, uniform_segments=d.uni, limits=R.LIMITS_OF[r], clearance=R.CLEARANCE,
                                       max_move=MOVE)
    # (the coefficients of the invalid trajectory: the host entry hands back zeros, the device entry leaves the test's zeroed buffer alone)
    for k, v in zip(OUT_KEYS, got):
        assert res[k].tobytes() == v.tobytes(), k


@pytest.mark.parametrize("r,kind", [(3, "ragged"), (4, "uniform")], ids=["r3-ragged", "r4-uniform"])
def test_lbfgs_max_iters_zero_is_the_plain_solve_after_the_projection(gpu_ctx, esdf, r, kind):
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    ok = valid_ids(d, bad)
    seg_ok = d.seg_traj != (-1 if bad is None else bad)
    t_min, t_max = 1.05 * d.T0[seg_ok].min(), 0.95 * d.T0[seg_ok].max()     # both bounds bind somewhere
    z = d.lbfgs(esdf, max_iters=0, t_min=t_min, t_max=t_max)
    T_want = np.where(seg_ok, np.minimum(np.maximum(d.T0, t_min), t_max), d.T0)
    assert z["wp"].tobytes() == d.wp0.tobytes() and z["T"].tobytes() == T_want.tobytes()
    assert np.any(T_want != d.T0)
    plain, st_plain = d.solve(d.up(d.wp0), d.up(T_want))
    assert z["coeff"].tobytes() == plain.cpu().numpy().tobytes() and np.array_equal(z["status"], st_plain.cpu().numpy())
    assert np.array_equal(z["obj"][ok, 0], z["obj"][ok, 1]) and np.all(z["acc"] == 0)
    pen = d.flight(esdf, d.up(T_want), plain, st_plain, want=("peak", "min_dist", "outside"))
    assert pen["peak"].tobytes() == z["peak"].tobytes() and pen["min_dist"].tobytes() == z["md"].tobytes() and np.array_equal(pen["outside"], z["outside"])
    # without binding bounds the start objective is that of the default run
    z2 = d.lbfgs(esdf, max_iters=0)
    assert z2["T"].tobytes() == d.T0.tobytes() and np.array_equal(z2["obj"][ok, 0], res["obj"][ok, 0])


@pytest.mark.parametrize("r,kind", KINDS, ids=IDS)
def test_lbfgs_start_and_first_trial_are_those_of_the_gradient_entry(gpu_ctx, esdf, r, kind):
    """objective_out[:, 0] with identical shared parameters, and EVERY output at max_iters = 1: the first trial is the gradient entry's."""
    d, res, _ = run_of(gpu_ctx, esdf, r, kind)
    old = d.optimize(esdf)
    assert res["obj"][:, 0].tobytes() == old["obj"][:, 0].tobytes()
    one, old_one = d.lbfgs(esdf, max_iters=1), d.optimize(esdf, max_iters=1)
    for k in OUT_KEYS:
        assert one[k].tobytes() == old_one[k].tobytes(), k
    assert np.any(one["acc"] == 1)


def test_lbfgs_optional_outputs_may_be_null(gpu_ctx, esdf):
    d, res, _ = run_of(gpu_ctx, esdf, 4, "uniform")
    part = d.lbfgs(esdf, null=("status", "acc", "peak", "md", "outside"))
    for k in ("wp", "T", "coeff", "obj"):
        assert part[k].tobytes() == res[k].tobytes(), k
    part = d.lbfgs(esdf, null=("peak", "outside"))
    for k in ("wp", "T", "coeff", "obj", "status", "acc", "md"):
        assert part[k].tobytes() == res[k].tobytes(), k


@pytest.mark.parametrize("params", [dict(memory=1), dict(memory=16), dict(max_backtracks=1)], ids=["memory1", "memory16", "backtracks1"])
@pytest.mark.parametrize("r,kind", [(3, "ragged"), (4, "uniform11")], ids=["r3-ragged", "r4-uniform11"])
def test_lbfgs_memory_edge_cases_meet_the_invariants(gpu_ctx, esdf, r, kind, params):
    """One pair, the most pairs the entry takes, and a reset after every rejected quasi-Newton trial."""
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    P = defaults()
    got = d.lbfgs(esdf, **params)
    check_invariants(d, got, bad, esdf, P.max_iters, P.t_min, P.t_max)
    again = d.lbfgs(esdf, **params)
    for k in OUT_KEYS:
        assert got[k].tobytes() == again[k].tobytes(), k
    assert got["obj"][:, 0].tobytes() == res["obj"][:, 0].tobytes()
    ok = valid_ids(d, bad)
    print(f"r={r} {kind} {params}: median f_result / f_start {np.median(got['obj'][ok, 1] / got['obj'][ok, 0]):.4f} (defaults "
          f"{np.median(res['obj'][ok, 1] / res['obj'][ok, 0]):.4f}), accepted {got['acc'][ok].min()} .. {got['acc'][ok].max()}")


# ---------------------------------------------------------------------------------------------------
# against the reference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,kind", SCIPY_KINDS, ids=SCIPY_IDS)
def test_lbfgs_objective_and_diagnostics_vs_reference(gpu_ctx, esdf, oracle, r, kind):
    """f, the peaks, min_dist and outside at the start and at the returned point: the oracle's solve + the longdouble penalties."""
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    start = d.lbfgs(esdf, max_iters=0)
    worst_f, worst_d, worst_p = 0.0, 0.0, 0.0
    for t in valid_ids(d, bad):
        prob = G.problem_of(oracle, r, kind, original_index(t, bad))
        k0, k1, s0, s1 = int(d.so[t]) + t, int(d.so[t + 1]) + t, int(d.so[t]), int(d.so[t + 1])
        for got, q in ((start, prob.parts(prob.start_p, R.clamp_times(prob.start_T))), (res, prob.parts(res["wp"][k0:k1 + 1], res["T"][s0:s1]))):
            col = 0 if got is start else 1
            worst_f = max(worst_f, abs(got["obj"][t, col] - q["f"]) / q["f"])
            worst_d = max(worst_d, abs(got["md"][t] - q["min_dist"]) / max(abs(q["min_dist"]), W.RES))
            worst_p = max(worst_p, float(np.max(np.abs(got["peak"][t] - q["peak"]) / q["peak"])))
            assert q["outside"] == 0 and got["outside"][t] == 0
    print(f"r={r} {kind}: max rel err vs reference: objective {worst_f:.3e}, min_dist {worst_d:.3e}, peaks {worst_p:.3e}")
    assert worst_f <= 1e-9
    assert worst_d <= 1e-9
    assert worst_p <= 1e-9


@pytest.mark.parametrize("r,kind", SCIPY_KINDS, ids=SCIPY_IDS)
def test_lbfgs_vs_scipy_lbfgsb_and_vs_the_gradient_entry(gpu_ctx, esdf, r, kind):
    """Per trajectory the fraction of scipy's decrease left after the default 32 trials is within GAP_BOUND, and the worst of the batch is
    smaller than the worst uavqp_spacetime_optimize_device leaves after its 32 trials."""
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    P = defaults()
    assert P.max_iters == Q.DEFAULT_MAX_ITERS == G.defaults().max_iters
    old = d.optimize(esdf)
    golden = json.load(open(G.GOLDEN))[f"r{r}-{kind}"]
    gaps, gaps_old = [], []
    for t in valid_ids(d, bad):
        rec = golden[original_index(t, bad)]
        f_start, f_scipy = res["obj"][t, 0], rec["f_scipy"]
        assert abs(f_start - rec["f_start"]) <= 1e-9 * f_start, "the recorded results belong to other cases"
        assert rec["outside"] == 0
        assert f_start > 1.5 * f_scipy, "the case has no decrease to speak of"
        gaps.append((res["obj"][t, 1] - f_scipy) / (f_start - f_scipy))
        gaps_old.append((old["obj"][t, 1] - f_scipy) / (f_start - f_scipy))
    worst, worst_old = max(gaps), max(gaps_old)
    print(f"r={r} {kind}: {len(gaps)} trajectories at max_iters = {P.max_iters}: worst gap {worst:.3e} (trajectory {int(np.argmax(gaps))}; bound "
          f"{GAP_BOUND:.3e}), the gradient entry's worst gap {worst_old:.3e}; median {np.median(gaps):.3e} against {np.median(gaps_old):.3e}")
    assert len(gaps) == d.n - (0 if bad is None else 1), "no trajectory is left out except the designed invalid one"
    for t, gap in zip(valid_ids(d, bad), gaps):
        assert gap <= GAP_BOUND, f"r={r} {kind} trajectory {t}: gap {gap:.3e}"
    assert worst < worst_old


@pytest.mark.parametrize("r,kind", SCIPY_KINDS, ids=SCIPY_IDS)
def test_lbfgs_penalised_trajectories_end_slower_and_farther_away(gpu_ctx, esdf, r, kind):
    """The three comparisons of tests/test_gpu_spacetime.py, all three runs at 64 trials."""
    d, _, bad = run_of(gpu_ctx, esdf, r, kind)
    ok = [t for t in valid_ids(d, bad)]
    inner = np.array([int(d.so[t + 1] - d.so[t]) > 1 for t in ok])
    n = Q.FEASIBILITY_ITERS
    assert n == 64
    res = d.lbfgs(esdf, max_iters=n)
    nolim = d.lbfgs(esdf, max_iters=n, limits=dict(weight_v=0.0, weight_a=0.0))
    noclr = d.lbfgs(esdf, max_iters=n, clearance=dict(weight=0.0))
    over = nolim["peak"][ok] > 1.0
    close = (noclr["md"][ok] < R.CLEARANCE["d_safe"]) & inner
    print(f"r={r} {kind}: {np.count_nonzero(over.any(axis=1))} of {len(ok)} exceed a limit without the limit penalty; worst peaks v / a "
          f"{nolim['peak'][ok].max(axis=0)} -> {res['peak'][ok].max(axis=0)}; {np.count_nonzero(close)} come closer than d_safe without the "
          f"clearance penalty, smallest distance {noclr['md'][ok].min():.3f} -> {res['md'][ok].min():.3f}")
    assert np.count_nonzero(over.any(axis=1)) * 2 >= len(ok), "fewer than half of the trajectories exceed a limit without the penalty"
    assert np.all(res["peak"][ok][over] < nolim["peak"][ok][over])
    assert np.count_nonzero(close) * 2 >= len(ok)
    assert np.all(res["md"][ok][close] > noclr["md"][ok][close])
    assert np.all(res["outside"][ok] == 0) and np.all(nolim["outside"][ok] == 0) and np.all(noclr["outside"][ok] == 0)


# ---------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------
def test_lbfgs_invalid_arguments_are_refused(gpu_ctx, esdf):
    d = Dev(gpu_ctx, R.uniform_cases(3), True)
    rg = Dev(gpu_ctx, R.cases(3), False)
    inf, nan = math.inf, math.nan
    for bad in (dict(max_iters=-1), dict(smooth_weight=-1.0), dict(smooth_weight=inf), dict(smooth_weight=nan), dict(time_weight=0.0),
                dict(time_weight=-1.0), dict(time_weight=inf), dict(time_weight=nan), dict(t_min=0.0), dict(t_min=-1.0), dict(t_min=nan),
                dict(t_min=2.0, t_max=1.0), dict(t_max=inf), dict(t_max=nan), dict(max_move=0.0), dict(max_move=-1.0), dict(max_move=nan),
                dict(initial_step_move=0.0), dict(initial_step_move=inf), dict(initial_step_log=0.0), dict(initial_step_log=inf),
                dict(initial_step_log=nan), dict(armijo_c=0.0), dict(armijo_c=1.0), dict(shrink=0.0), dict(shrink=1.0), dict(grow=0.5),
                dict(grow=inf),
                dict(memory=0), dict(memory=17), dict(max_backtracks=0), dict(max_backtracks=65), dict(curvature_eps=-1e-3),
                dict(curvature_eps=1.0), dict(curvature_eps=nan)):
        with pytest.raises(U.UavqpError):
            d.lbfgs(esdf, **bad)
    with pytest.raises(ValueError):
        d.lbfgs(esdf, struct_size=4)
    with pytest.raises(ValueError):
        d.lbfgs(esdf, no_such_field=1.0)
    pp, cp, lp = defaults(), _lib.ClearanceParams(), _lib.LimitParams()
    _lib.lib().uavqp_default_clearance_params(ctypes.byref(cp))
    _lib.lib().uavqp_default_limit_params(ctypes.byref(lp))
    d_T = d.up(d.T0)
    args = lambda p: (gpu_ctx._h, 3, d.n, d.uni, d.mmax, d.total, None, d.up(d.wp0).data_ptr(), d_T.data_ptr(), d.d_bc.data_ptr(), esdf.handle,
                      ctypes.byref(lp), ctypes.byref(cp), p, d.zeros(3 * 6 * d.total).data_ptr(), None, d.zeros((d.n, 2)).data_ptr(), None, None,
                      None, None)
    pp.max_iters = 2
    assert _lib.lib().uavqp_spacetime_lbfgs_device(*args(ctypes.byref(pp))) == _lib.UAVQP_OK
    gpu_ctx.synchronize()
    pp.struct_size = ctypes.sizeof(_lib.SpacetimeParams)
    assert _lib.lib().uavqp_spacetime_lbfgs_device(*args(ctypes.byref(pp))) == _lib.UAVQP_ERR_INVALID_ARG   # the other entry's struct
    old = G.defaults()
    assert _lib.lib().uavqp_spacetime_lbfgs_device(*args(ctypes.cast(ctypes.byref(old), ctypes.POINTER(_lib.SpacetimeLbfgsParams)))) \
        == _lib.UAVQP_ERR_INVALID_ARG
    assert _lib.lib().uavqp_spacetime_lbfgs_device(*args(None)) == _lib.UAVQP_ERR_INVALID_ARG               # NULL params
    for bad in (dict(d_safe=0.0), dict(weight=-1.0), dict(samples_per_seg=0)):
        with pytest.raises(U.UavqpError):
            d.lbfgs(esdf, clearance=bad)
    for bad in (dict(v_max=0.0), dict(a_max=-1.0), dict(weight_v=-1.0), dict(weight_a=inf), dict(samples_per_seg=0)):
        with pytest.raises(U.UavqpError):
            d.lbfgs(esdf, limits=bad)
    with pytest.raises(U.UavqpError):
        d.lbfgs(None)                                                  # a NULL map
    fresh = EsdfMap(gpu_ctx, (4, 4, 4), (0.0, 0.0, 0.0), 0.5)
    with pytest.raises(U.UavqpError):
        d.lbfgs(fresh)                                                 # a map that was never updated
    fresh.close()
    with pytest.raises(U.UavqpError):
        rg.lbfgs(esdf, so=False)                                       # ragged without offsets
    with pytest.raises(U.UavqpError):
        d.lbfgs(esdf, total=d.total + 1)                               # a wrong total_segments
    with pytest.raises(U.UavqpError):
        d.lbfgs(esdf, null=("obj",))                                   # objective_out is not optional
    # every bound that is allowed: max_move = INFINITY, t_min = t_max, smooth_weight = 0, grow = 1, curvature_eps = 0, max_backtracks = 64
    res = d.lbfgs(esdf, max_move=inf, max_iters=4, smooth_weight=0.0, grow=1.0, curvature_eps=0.0, max_backtracks=64)
    assert np.all(res["status"] == U.UAVQP_SOLVED) and np.all(res["obj"][:, 1] <= res["obj"][:, 0])
    res = d.lbfgs(esdf, max_iters=4, t_min=1.0, t_max=1.0)
    assert np.all(res["T"] == 1.0) and np.all(res["status"] == U.UAVQP_SOLVED)
