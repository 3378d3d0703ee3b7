"""CPU: the contract of the swarm optimiser (no compute calls): header, binding and library agree on the three new symbols and on
uavqp_swarm_opt_params; the facades exist and refuse unknown fields; the TOTAL gradient of the reference of tests/swarm_opt_reference.py
(SwarmProblem: the per-vehicle adjoint of tests/spacetime_reference.py fed with the sum of the flight penalty's and the swarm penalty's
coefficient gradients) is pinned against central differences of its f_g in EVERY duration, EVERY departure and random waypoint
directions, before any GPU run; and the recorded results of tests/golden/swarm_opt_scipy.json belong to the cases and show what the GPU
tests presuppose.

Criterion of the gradient test (that of tests/test_swarm_contract.py): the error relative to the largest component of the block, compared
with the finite-difference scheme's own error, estimated at run time (Richardson: h against h / 2).  Sample-distance rule (the same
file): the seeds below are the first from 1 at which every clock sample is at least ten steps from a knot, from its vehicle's departure
and from its arrival, every penalised pair ten steps inside rho2 = 1 and Phi_swarm > 0 -- and, for the clearance part of the flight
penalty (tests/test_spacetime_contract.py), no sample within ten steps of a face of the trilinear query or of d = d_safe.  The test
asserts that this is so, from the reference alone."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import spacetime_reference as R
import swarm_opt_reference as O
import swarm_reference as S
import waypoint_opt_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "swarm_opt_scipy.json")
NEW = ("uavqp_default_swarm_opt_params", "uavqp_swarm_optimize_device", "uavqp_swarm_optimize_host")
H = 1e-4   # seconds (durations, departures) and metres (along a waypoint direction)
FLIGHT = 4.0   # s: faster than the batches of the GPU tests, so that the limit part is active in most vehicles
# (r, segments per vehicle): swarms of 2, 3 and 5, M = 1 among them
CASES = [(3, (1, 3)), (3, (2, 1, 4)), (3, (3, 1, 2, 5, 2)), (4, (3, 1)), (4, (1, 2, 3)), (4, (2, 4, 1, 3, 5))]
SEED = {(3, (1, 3)): 1, (3, (2, 1, 4)): 1, (3, (3, 1, 2, 5, 2)): 1, (4, (3, 1)): 1, (4, (1, 2, 3)): 1, (4, (2, 4, 1, 3, 5)): 1}


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
    assert len(_lib.lib().uavqp_swarm_optimize_device.argtypes) == 26 and len(_lib.lib().uavqp_swarm_optimize_host.argtypes) == 25


def test_params_struct_matches_the_header_and_defaults_are_those_of_the_issue():
    from uav_motion_planning_amd import _lib
    body = re.search(r"typedef struct uavqp_swarm_opt_params \{(.*?)\} uavqp_swarm_opt_params;", header_text(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s*(int32_t|double)\s+([a-z_]+);", body, flags=re.M)
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.SwarmOptParams._fields_)
    shared = [n for n, _ in _lib.SpacetimeParams._fields_]
    assert [n for _, n in fields] == shared + ["start_window", "initial_step_start"]
    p, s = _lib.SwarmOptParams(), _lib.SpacetimeParams()
    _lib.lib().uavqp_default_swarm_opt_params(ctypes.byref(p))   # callable without a GPU
    _lib.lib().uavqp_default_spacetime_params(ctypes.byref(s))
    assert p.struct_size == ctypes.sizeof(_lib.SwarmOptParams) == ctypes.sizeof(_lib.SpacetimeParams) + 16
    for n in shared[1:]:
        assert getattr(p, n) == getattr(s, n), n
    assert (p.start_window, p.initial_step_start) == (0.0, 0.1)
    assert p.max_iters == O.DEFAULT_MAX_ITERS and p.max_iters in O.STEPS
    for k in ("start_window", "initial_step_start", "initial_step_move", "initial_step_log", "armijo_c", "shrink", "grow", "t_min", "t_max"):
        assert O.PARAMS[k] == getattr(p, k), k                  # the reference starts from the same defaults (max_move is the tests' own)
    _lib.lib().uavqp_default_swarm_opt_params(None)             # a NULL is ignored


def test_python_and_cpp_facades_carry_the_new_methods():
    import uav_motion_planning_amd as U
    for name in ("swarm_optimize_device", "swarm_optimize_host", "_swarm_opt_params"):
        assert callable(getattr(U.Context, name))
    assert callable(U.TrajOptimizer.optimizeSwarm)
    cpp = open(os.path.join(ROOT, "uav_motion_planning_amd", "cpp", "traj_optimizer.h")).read()
    assert "bool optimizeSwarm(" in cpp and "uavqp_swarm_optimize_host(" in cpp
    assert U.Context._swarm_opt_params(dict(start_window=0.5, max_iters=7)).start_window == 0.5
    for bad in (dict(no_such_field=1.0), dict(struct_size=112), dict(memory=4)):
        with pytest.raises(ValueError):
            U.Context._swarm_opt_params(bad)
    opt = U.TrajOptimizer(order=3)
    opt.setWaypoints(np.zeros((3, 3)), n_waypoints=3)
    opt.setCorridor(np.zeros((3, 3)), np.ones((3, 3)))
    with pytest.raises(ValueError):
        opt.optimizeSwarm(None)                                 # corridor problems are out of scope: refused before any device call
    opt.setCorridor(None, None)
    with pytest.raises(ValueError):
        opt.optimizeSwarm(None, no_such_field=1.0)
    with pytest.raises(ValueError):
        opt.optimizeSwarm(None, swarm=dict(no_such_field=1.0), max_iters=1)


def build_case(oracle, r, Ms, seed):
    rng = np.random.default_rng(100000 * r + 1000 * len(Ms) + seed)
    wps, Ts, starts = S.scene(rng, list(Ms), centre=O.CENTRE, radius=O.RADIUS, flight=FLIGHT)
    bcs = [rng.uniform(-0.3, 0.3, size=(2, r - 1, 3)) for _ in Ms]     # non-zero boundary derivatives
    return O.SwarmProblem(oracle, r, wps, Ts, bcs, starts, smooth_weight=0.7, time_weight=30.0, swarm=dict(n_samples=60))


def preconditions(q):
    """-> the list of what the sample-distance rule finds wrong with the point (empty: the point may be differenced)"""
    sw, bad = q["swarm"], []
    if not float(sw["phi"]) > 0.0:
        bad.append("the swarm penalty is not active")
    if not sw["knot_margin"] >= 10.0 * H:
        bad.append("a clock sample sits on a knot")
    if not sw["hold_margin"] >= 10.0 * H:
        bad.append("a clock sample sits on a departure or an arrival")
    if not sw["rho_gap"] >= 10.0 * H:
        bad.append("a penalised pair sits on rho2 = 1")
    for v in q["veh"]:
        if v["outside"] != 0:
            bad.append("a sample lies outside the map")
        if float(v["clr"]["phi"][0]) > 0.0 and not (float(v["clr"]["margin"]) > 10.0 * H / W.RES and float(v["clr"]["gap"]) > 10.0 * H):
            bad.append("a clearance sample sits on a face of the trilinear query or on d = d_safe")
    if not any(float(v["lim"]["phi"][0]) > 0.0 for v in q["veh"]):
        bad.append("the limit penalty is not active in any vehicle")
    return bad


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"r{c[0]}-A{len(c[1])}")
def test_total_gradient_vs_central_differences_of_the_reference_objective(oracle, case):
    r, Ms = case
    prob = build_case(oracle, r, Ms, SEED[case])
    ps, Ts, st = prob.start()
    q, gps, gTs, gs = prob.grad(ps, Ts, st)
    assert preconditions(q) == []
    A = len(Ms)
    rng = np.random.default_rng(7)
    dirs = []
    for _ in range(4):
        d = [np.zeros_like(p) for p in ps]
        for b, M in enumerate(Ms):
            d[b][1:M] = rng.standard_normal((M - 1, 3))      # interior waypoints only: the end knots are not variables
        dirs.append(d)

    def central(h):
        fT, fs, fd = [np.zeros(M) for M in Ms], np.zeros(A), np.zeros(len(dirs))
        for i in range(A):
            for l in range(Ms[i]):
                up, dn = [T.copy() for T in Ts], [T.copy() for T in Ts]
                up[i][l] += h
                dn[i][l] -= h
                fT[i][l] = (prob.f(ps, up, st) - prob.f(ps, dn, st)) / (up[i][l] - dn[i][l])
            up, dn = st.copy(), st.copy()
            up[i] += h
            dn[i] -= h
            fs[i] = (prob.f(ps, Ts, up) - prob.f(ps, Ts, dn)) / (up[i] - dn[i])
        for k, d in enumerate(dirs):
            fd[k] = (prob.f([p + h * e for p, e in zip(ps, d)], Ts, st) - prob.f([p - h * e for p, e in zip(ps, d)], Ts, st)) / (2.0 * h)
        return np.concatenate(fT), fs, fd

    got = (np.concatenate(gTs), gs, np.array([sum(float(np.sum(g * e)) for g, e in zip(gps, d)) for d in dirs]))
    one, two = central(H), central(H / 2)
    msg = f"r={r} Ms={Ms}: f_g = {q['f']:.4e} (swarm {q['phi_swarm']:.3e})"
    for name, g, f1, f2 in zip(("durations", "departures", "waypoint directions"), got, one, two):
        scale = np.max(np.abs(g))
        assert scale > 0.0
        rich, err = float(np.max(np.abs(f1 - f2)) / scale), float(np.max(np.abs(f2 - g)) / scale)
        msg += f"; {name} |fd - grad| / max = {err:.3e} (Richardson {rich:.3e})"
        assert rich < 1e-5, f"{name}: the finite-difference step is badly chosen ({msg})"
        assert err <= 10.0 * rich, msg
    print(msg)


def test_the_transcription_never_increases_f_and_keeps_its_bounds(oracle):
    b = O.batch_of(3, "ragged")
    prob = O.SwarmProblem.of_batch(oracle, b, 2)
    ps, Ts, st = prob.start()
    run = O.iterate_swarm(prob, 12, max_move=0.2, t_min=0.5, t_max=2.5, start_window=0.1)
    hist = np.concatenate([[run["f_start"]], run["history"]])
    assert np.all(np.diff(hist) <= 0.0) and run["accepted"] > 0 and run["f"] < run["f_start"]
    assert run["f_start"] == prob.f(ps, [np.minimum(np.maximum(T, 0.5), 2.5) for T in Ts], st)
    for p, p0, T in zip(run["p"], ps, run["T"]):
        assert np.array_equal(p[[0, -1]], p0[[0, -1]]) and np.all(p >= p0 - 0.2) and np.all(p <= p0 + 0.2)
        assert np.all(T >= 0.5) and np.all(T <= 2.5)
    assert np.all(run["start"] >= st - 0.1) and np.all(run["start"] <= st + 0.1) and np.any(run["start"] != st)
    fixed = O.iterate_swarm(prob, 4)
    assert np.array_equal(fixed["start"], st)                  # start_window = 0, the default: the departures do not move


def test_the_stored_gap_is_what_the_transcription_gives(oracle):
    """GAP_AT_DEFAULT on the swarm it was found at, against the recorded optimum (tools/swarm_opt_convergence.py runs scipy on all of them)"""
    r, kind, g = O.GAP_CASE
    rec = json.load(open(GOLDEN))[f"r{r}-{kind}"][g]
    run = O.iterate_swarm(O.SwarmProblem.of_batch(oracle, O.batch_of(r, kind), g), O.DEFAULT_MAX_ITERS)
    gap = (run["f"] - rec["f_scipy"]) / (run["f_start"] - rec["f_scipy"])
    print(f"r={r} {kind} swarm {g}: f_start {run['f_start']:.6e} f_scipy {rec['f_scipy']:.6e} f after {O.DEFAULT_MAX_ITERS} trials {run['f']:.6e} gap {gap:.4e}")
    assert abs(gap - O.GAP_AT_DEFAULT) <= 0.02 * O.GAP_AT_DEFAULT
    assert abs(gap - rec["gap"][str(O.DEFAULT_MAX_ITERS)]) <= 1e-6
    worst = max(q["gap"][str(O.DEFAULT_MAX_ITERS)] for recs in json.load(open(GOLDEN)).values() for q in recs)
    assert abs(worst - O.GAP_AT_DEFAULT) <= 0.02 * O.GAP_AT_DEFAULT


def test_the_recorded_optima_belong_to_the_cases_and_show_what_the_gpu_tests_presuppose(oracle):
    """tests/golden/swarm_opt_scipy.json (tools/swarm_opt_convergence.py --write-golden): one record per swarm of the four compared
    batches; f_start of the cases as they are built today, to 1e-9; no sample outside the map; and in at least half of the recorded
    swarms the run with swarm weight = 0 comes closer than d_safe and the penalised run ends with a larger smallest separation."""
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == ["r3-ragged", "r3-uniform", "r4-ragged", "r4-uniform"]
    for key, recs in golden.items():
        r, kind = int(key[1]), key[3:]
        b = O.batch_of(r, kind)
        assert len(recs) == b["group_offsets"].size - 1
        apart = 0
        for g, rec in enumerate(recs):
            prob = O.SwarmProblem.of_batch(oracle, b, g)
            assert rec["Ms"] == [v.M for v in prob.veh]
            f_start = prob.f(*prob.start())
            assert abs(rec["f_start"] - f_start) <= 1e-9 * f_start, (key, g)
            assert rec["outside"] == 0 and rec["f_scipy"] < rec["f_start"]
            apart += rec["noswarm_min_sep"] < O.SWARM["d_safe"] and rec["min_sep"] > rec["noswarm_min_sep"]
        assert 2 * apart >= len(recs), (key, apart)
