"""CPU: the contract of the joint optimiser with limited-memory BFGS directions (no compute calls): header, binding and library agree on
the three new symbols and on uavqp_spacetime_lbfgs_params; both facades carry the new methods; the numpy transcription of the method
(tests/spacetime_lbfgs_reference.py, written from the header text) never increases f and keeps its bounds; the stored
GAP_LBFGS_AT_DEFAULT is what it gives; on each of the four scipy batches it leaves less after 32 trials than projected gradient descent
does, and over all of them at most HALF of R.GAP_AT_DEFAULT -- the condition the method was accepted on.

The per-batch comparison runs every trajectory of the batch through BOTH transcriptions for 32 trials (tools/spacetime_convergence.py
--method lbfgs prints the same figures; DESIGN.md sections 5.20 and 5.21 hold the tables)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import spacetime_lbfgs_reference as Q
import spacetime_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("uavqp_default_spacetime_lbfgs_params", "uavqp_spacetime_lbfgs_device", "uavqp_spacetime_lbfgs_host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "spacetime_scipy.json")
BATCHES = [(3, "ragged"), (3, "uniform"), (4, "ragged"), (4, "uniform")]


def header_text():
    return open(os.path.join(ROOT, "include", "uavqp.h")).read()


def test_header_binding_and_library_agree_on_the_new_entries():
    import __graft_entry__ as g
    g.build()
    from uav_motion_planning_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    declared = set(re.findall(r"\b(uavqp_[a-z_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, f"{name} not declared in include/uavqp.h"
        assert name in _lib.SYMBOLS, f"{name} missing from _lib.SYMBOLS"
        assert hasattr(L, name), f"{name} not exported by libuavqp.so"
        assert getattr(_lib.lib(), name).argtypes is not None, f"{name} has no argtypes"
    # the two entries take the argument lists of the entries they stand beside
    old, new = _lib.lib().uavqp_spacetime_optimize_device.argtypes, _lib.lib().uavqp_spacetime_lbfgs_device.argtypes
    assert [a for a in old if a is not ctypes.POINTER(_lib.SpacetimeParams)] == [a for a in new if a is not ctypes.POINTER(_lib.SpacetimeLbfgsParams)]
    assert len(old) == len(new) and len(_lib.lib().uavqp_spacetime_optimize_host.argtypes) == len(_lib.lib().uavqp_spacetime_lbfgs_host.argtypes)
    # the old entry's comment points to the new one where it used to list quasi-Newton directions as out of scope
    assert "uavqp_spacetime_lbfgs_device below" in header_text()


def test_params_struct_matches_the_header_and_defaults_are_those_of_the_issue():
    from uav_motion_planning_amd import _lib
    body = re.search(r"typedef struct uavqp_spacetime_lbfgs_params \{(.*?)\} uavqp_spacetime_lbfgs_params;", header_text(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s*(int32_t|double)\s+([a-z_]+);", body, flags=re.M)
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.SpacetimeLbfgsParams._fields_)
    assert [n for _, n in fields] == ["struct_size", "max_iters", "memory", "max_backtracks", "smooth_weight", "time_weight", "t_min", "t_max",
                                      "max_move", "initial_step_move", "initial_step_log", "armijo_c", "shrink", "grow", "curvature_eps"]
    p, s = _lib.SpacetimeLbfgsParams(), _lib.SpacetimeParams()
    _lib.lib().uavqp_default_spacetime_lbfgs_params(ctypes.byref(p))   # callable without a GPU
    _lib.lib().uavqp_default_spacetime_params(ctypes.byref(s))
    assert p.struct_size == ctypes.sizeof(_lib.SpacetimeLbfgsParams) != ctypes.sizeof(_lib.SpacetimeParams)
    assert (p.max_iters, p.memory, p.max_backtracks, p.curvature_eps) == (32, 8, 6, 1e-10)
    for name, _ in _lib.SpacetimeParams._fields_:
        if name != "struct_size":
            assert getattr(p, name) == getattr(s, name), name           # every shared field takes the other entry's default
    assert (p.max_iters, p.memory, p.max_backtracks, p.curvature_eps) == (Q.DEFAULT_MAX_ITERS, Q.PARAMS["memory"], Q.PARAMS["max_backtracks"],
                                                                         Q.PARAMS["curvature_eps"])
    _lib.lib().uavqp_default_spacetime_lbfgs_params(None)               # a NULL is ignored


def test_python_and_cpp_facades_carry_the_new_methods():
    import uav_motion_planning_amd as U
    for name in ("spacetime_lbfgs_device", "spacetime_lbfgs_host"):
        assert callable(getattr(U.Context, name))
    assert callable(U.TrajOptimizer.optimizeTrajectoryLbfgs)
    cpp = open(os.path.join(ROOT, "uav_motion_planning_amd", "cpp", "traj_optimizer.h")).read()
    assert "bool optimizeTrajectoryLbfgs(" in cpp and "const uavqp_spacetime_lbfgs_params* params = nullptr" in cpp
    with pytest.raises(ValueError):
        U.Context._spacetime_lbfgs_params(dict(no_such_field=1.0))
    assert U.Context._spacetime_lbfgs_params(dict(memory=4)).memory == 4
    opt = U.TrajOptimizer(order=3)
    opt.setWaypoints(np.zeros((3, 3)), n_waypoints=3)
    opt.setCorridor(np.zeros((3, 3)), np.ones((3, 3)))
    with pytest.raises(ValueError):
        opt.optimizeTrajectoryLbfgs(None)                            # corridor problems are out of scope: refused before any device call
    opt.setCorridor(None, None)
    with pytest.raises(ValueError):
        opt.optimizeTrajectoryLbfgs(None, no_such_field=1.0)


def problem_of(oracle, r, kind, t):
    wp, T, bc = R.split(R.batch_of(r, kind), t)
    return R.Problem(oracle, r, wp, T, bc)


@pytest.mark.parametrize("params", [{}, dict(memory=1), dict(max_backtracks=1)], ids=["defaults", "memory1", "backtracks1"])
def test_the_transcription_never_increases_f_and_keeps_its_bounds(oracle, params):
    b = R.cases(3)
    for t in (1, 4, 11):                                  # M = 3, M = 6, and M = 1: the duration alone
        wp, T, bc = R.split(b, t)
        prob = R.Problem(oracle, 3, wp, T, bc)
        # the bounds of tests/test_spacetime_contract.py: the upper bound binds at the start, so the projection comes first
        t_min, t_max = 0.5 * T.min(), (0.9 if T.size > 1 else 3.0) * T.max()
        run = Q.iterate_lbfgs(prob, 24, max_move=0.2, t_min=t_min, t_max=t_max, **params)
        hist = np.concatenate([[run["f_start"]], run["history"]])
        assert np.all(np.diff(hist) <= 0.0)
        assert run["f_start"] == prob.f(wp, np.minimum(T, t_max))
        assert np.array_equal(run["p"][[0, -1]], wp[[0, -1]])
        assert np.all(run["p"] >= wp - 0.2) and np.all(run["p"] <= wp + 0.2)
        assert np.all(run["T"] >= t_min) and np.all(run["T"] <= t_max)
        assert run["accepted"] > 0 and run["f"] < run["f_start"]
        assert run["stored"] > 0, "no pair was ever stored: the run was gradient descent"
        if T.size == 1:
            assert np.array_equal(run["p"], wp) and run["T"][0] != T[0]
        # the first trial is that of the projected-gradient transcription
        first, old = Q.iterate_lbfgs(prob, 1, max_move=0.2, t_min=t_min, t_max=t_max, **params), R.iterate(prob, 1, max_move=0.2, t_min=t_min, t_max=t_max)
        assert np.array_equal(first["p"], old["p"]) and np.array_equal(first["T"], old["T"]) and first["f"] == old["f"]


def gap_of(oracle, golden, r, kind, t, iterate, iters):
    rec = golden[f"r{r}-{kind}"][t]
    run = iterate(problem_of(oracle, r, kind, t), iters)
    assert abs(run["f_start"] - rec["f_start"]) <= 1e-9 * rec["f_start"], "the recorded results belong to other cases"
    return (run["f"] - rec["f_scipy"]) / (run["f_start"] - rec["f_scipy"])


def test_the_stored_gap_is_what_the_transcription_gives(oracle):
    """GAP_LBFGS_AT_DEFAULT on the trajectory it was found at, against the recorded scipy optimum (tests/test_spacetime_contract.py
    recomputes that record for R.GAP_CASE, the same trajectory)."""
    r, kind, t = Q.GAP_LBFGS_CASE
    gap = gap_of(oracle, json.load(open(GOLDEN)), r, kind, t, Q.iterate_lbfgs, Q.DEFAULT_MAX_ITERS)
    print(f"r={r} {kind} t={t}: gap after {Q.DEFAULT_MAX_ITERS} trials {gap:.4e} (stored {Q.GAP_LBFGS_AT_DEFAULT:.4e})")
    assert abs(gap - Q.GAP_LBFGS_AT_DEFAULT) <= 0.02 * Q.GAP_LBFGS_AT_DEFAULT


@pytest.mark.parametrize("r,kind", BATCHES, ids=[f"r{r}-{k}" for r, k in BATCHES])
def test_lbfgs_leaves_less_than_gradient_descent_on_every_batch_and_half_overall(oracle, r, kind):
    """Per batch: the worst gap of the new transcription over ALL trajectories after 32 trials is below gradient descent's worst, taken as
    the largest of R.iterate's gaps over all trajectories too (32 trials each: a second or two per batch).  Overall (the headline condition):
    at most R.GAP_AT_DEFAULT / 2."""
    golden = json.load(open(GOLDEN))
    n = len(golden[f"r{r}-{kind}"])
    new = [gap_of(oracle, golden, r, kind, t, Q.iterate_lbfgs, Q.DEFAULT_MAX_ITERS) for t in range(n)]
    old = [gap_of(oracle, golden, r, kind, t, R.iterate, R.DEFAULT_MAX_ITERS) for t in range(n)]
    print(f"r={r} {kind}: worst gap after 32 trials {max(new):.3e} (trajectory {int(np.argmax(new))}), gradient descent {max(old):.3e} "
          f"(trajectory {int(np.argmax(old))})")
    assert Q.DEFAULT_MAX_ITERS == R.DEFAULT_MAX_ITERS
    assert max(new) < max(old)
    assert max(new) <= R.GAP_AT_DEFAULT / 2.0
    assert max(new) <= Q.GAP_LBFGS_AT_DEFAULT * 1.02
