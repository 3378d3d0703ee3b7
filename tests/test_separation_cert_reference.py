"""CPU: the soundness of the reference the GPU tests compare against (tests/separation_cert_reference.py) against the mpmath truth, what the
coefficient difference buys (formation), nesting in the depth, the contract of the certificate in include/uavqp.h, and the conditions on
the inputs of tests/test_gpu_separation_cert.py.

Soundness has NO tolerance: lower <= truth at 64 instants of every depth-3 leaf and truth(witness) <= upper, in mpmath arithmetic.
The allowance of the other tests is the method's own, sqrt(3) max (G_i + G_j) + R of the pair that decides (about 1e-12 m here)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import separation_cert_reference as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = (0, 2, 5)


@functools.lru_cache(maxsize=None)
def small(r, downwash):
    from oracle import oracle
    oracle.build()
    b, clock = C.small_batch(r, downwash)
    co = C.solve(oracle, b)
    return b, clock, co, C.truth(r, b["so"], b["T"], co, group_offsets=b["go"], start=b["start"], **clock)


def sound(r, b, co, clock, tr, tag, depths=DEPTHS, **kw):
    bad, states = [], set()
    for depth in depths:
        ref = C.certificate(r, b["so"], b["T"], co, group_offsets=b["go"], start=b["start"], **dict(clock, depth=depth), **kw)
        bad += C.soundness_failures(ref, tr, C.taus(depth, clock["n_cells"], clock["clock_start"], clock["dt"]), f"{tag} depth={depth}")
        states |= ref["states"]
        gap = [float(tr[0][i] - ref["lower"][i]) for i in range(len(tr[0])) if tr[0][i] is not None]
        print(f"{tag} depth {depth}: truth - lower median {np.median(gap):.3g} m, max {np.max(gap):.3g} m")
    assert not bad, "\n".join(bad[:20])
    return states


@pytest.mark.parametrize("r,downwash", [(3, 1.0), (4, 1.5)])
def test_reference_is_sound_against_the_truth(r, downwash):
    """swarms of 2, 3, 5 and 1 vehicles, ragged M in 1..11 and M = 1, staggered departures: waiting, moving, arrived and straddling leaves"""
    b, clock, co, tr = small(r, downwash)
    Ms = np.diff(b["so"])
    assert Ms.min() == 1 and Ms.max() == 11
    states = sound(r, b, co, clock, tr, f"r={r}")
    assert states == {0, 1, 2, 3}, "moving, waiting, arrived and straddling leaves all occur"
    assert tr[0][sum(C.SMALL_SIZES) - 1] is None, "the swarm of one has no partner"


def test_a_leaf_that_straddles_several_knots_and_a_discontinuous_input(oracle):
    """T = 0.3 with dt = 1.0: every leaf of depth 0 straddles three knots; and the same swarm with a jump of 0.5 m put into one vehicle at
    a knot (pieces are closed: both values belong to the curve)"""
    r = 4
    b = C.make_batch(r, (3,), [9, 7, 8], seed=21, flight=2.5)
    b["T"][:] = 0.3
    co = C.solve(oracle, b)
    clock = dict(n_cells=3, clock_start=-0.2, dt=1.0, downwash=1.0, d_req=0.5)
    tr = C.truth(r, b["so"], b["T"], co, group_offsets=b["go"], start=b["start"], per_leaf=32, **clock)
    assert 3 in sound(r, b, co, clock, tr, "short segments", depths=(0, 2))
    jump = co.copy()
    jump[4 * 2 * r] += 0.5            # vehicle 0, axis x, segment 4, the constant coefficient
    K = C.knots(b["T"][:9], b["start"][0])
    tr = C.truth(r, b["so"], b["T"], jump, group_offsets=b["go"], start=b["start"], per_leaf=32, extra=(K[4], K[5]), **clock)
    sound(r, b, jump, clock, tr, "discontinuous", depths=(0, 2))


def formation():
    """two copies of one trajectory offset by (1, 0, 0); dyadic durations and dt, so that no leaf straddles"""
    r = 4
    rng = np.random.default_rng(4)
    T = np.array([0.5, 1.0, 1.5])
    c = rng.uniform(-1.0, 1.0, size=(3, 3, 2 * r))
    c2 = c.copy()
    c2[0, :, 0] += 1.0
    so = np.array([0, 3, 6], dtype=np.int32)
    return r, so, np.concatenate([T, T]), np.concatenate([c.ravel(), c2.ravel()]), dict(n_cells=8, clock_start=-0.5, dt=0.5, downwash=1.0, d_req=0.99)


def test_formation_is_certified_by_the_coefficient_difference_and_not_by_boxes():
    r, so, T, co, clock = formation()
    ref = C.certificate(r, so, T, co, depth=0, **clock)
    assert 3 not in ref["states"], "dyadic knots: no leaf straddles"
    assert np.all(np.abs(ref["lower"] - 1.0) <= ref["allow_lower"]) and np.all(np.abs(ref["upper"] - 1.0) <= ref["allow_upper"])
    assert np.all(ref["verdict"] & C.CERTIFIED) and ref["group_verdict"][0] & C.CERTIFIED
    box = C.certificate(r, so, T, co, depth=0, force_box=True, **clock)
    assert not np.any(box["verdict"] & C.CERTIFIED) and np.all(box["lower"] < 0.5), "the interval difference of two boxes loses the correlation"
    print(f"formation: lower {ref['lower'][0]!r} by coefficient differences, {box['lower'][0]!r} by boxes")


@pytest.mark.parametrize("r,downwash", [(3, 1.0), (4, 1.5)])
def test_bounds_nest_in_the_depth(r, downwash):
    """lower(depth + 1) >= lower(depth) and upper(depth + 1) <= upper(depth), each within the allowance"""
    b, clock, co, _ = small(r, downwash)
    prev = None
    for depth in range(5):
        ref = C.certificate(r, b["so"], b["T"], co, group_offsets=b["go"], start=b["start"], **dict(clock, depth=depth))
        if prev is not None:
            fin = np.isfinite(ref["lower"])
            allow = np.maximum(ref["allow_lower"], prev["allow_lower"]) + np.maximum(ref["allow_upper"], prev["allow_upper"])
            assert np.all(ref["lower"][fin] >= prev["lower"][fin] - allow[fin]), depth
            assert np.all(ref["upper"][fin] <= prev["upper"][fin] + allow[fin]), depth
        prev = ref


# -------------------------------------------------------------------------------------------- the inputs of the GPU test
@pytest.mark.parametrize("kind", sorted(C.GPU_KINDS))
def test_gpu_inputs_qualify(oracle, kind):
    """every class of verdict occurs; d_req is more than two allowances from every bound; `where` is compared on more than half of the vehicles (those whose
    runner-up is more than two allowances from the winner: pairs that hold still tie from leaf to leaf); no knot within 1e-9 s of a leaf end"""
    b = C.gpu_batch(kind)
    co = C.solve(oracle, b)
    r = b["r"]
    classes, moving = set(), False
    for depth, n_cells in C.GPU_CLOCKS:
        clock = C.gpu_clock(depth, n_cells)
        ref = C.certificate(r, b["so"], b["T"], co, group_offsets=b["go"], start=b["start"], **clock)
        assert C.two_allowances_away(ref, clock["d_req"]), (kind, depth, n_cells)
        assert ref["knot_margin"] > 1e-9, (kind, depth, n_cells)
        lo_ok, up_ok = C.where_comparable(ref)
        assert lo_ok.mean() > 0.5 and up_ok.mean() > 0.5, (kind, depth, n_cells, lo_ok.mean(), up_ok.mean())
        classes |= {C.state(int(w)) for w in ref["verdict"]}
        moving = moving or bool(np.any(ref["verdict"] & C.MOVING))
        one = sum(C.GPU_SIZES[:2])
        assert np.isinf(ref["lower"][one]) and ref["verdict"][one] & C.CERTIFIED and ref["where"][one].tolist() == [-1, 0, -1, 0]
    assert classes == {"certified", "violated", "undecided"} and moving


@pytest.mark.parametrize("r", [3, 4])
def test_full_swarm_input_qualifies(oracle, r):
    b = C.full_swarm_batch(r)
    ref = C.certificate(r, b["so"], b["T"], C.solve(oracle, b), group_offsets=b["go"], start=b["start"], **C.FULL_CLOCK)
    assert C.two_allowances_away(ref, C.FULL_CLOCK["d_req"]) and ref["knot_margin"] > 1e-9
    assert {C.state(int(w)) for w in ref["verdict"]} == {"violated", "undecided"}      # (128 paths through one centre: nothing to certify)


# ---------------------------------------------------------------------------------------------------------------- contract
def header():
    with open(os.path.join(ROOT, "include", "uavqp.h")) as fh:
        return fh.read()


def test_header_declares_the_entries_the_struct_and_the_bits():
    h = header()
    names = ("uavqp_default_separation_params", "uavqp_separation_certificate_device", "uavqp_separation_certificate_host")
    for name in names:
        assert re.search(rf"\b{name}\(", h), name
    for name, val in (("CERTIFIED", C.CERTIFIED), ("VIOLATED", C.VIOLATED), ("MOVING", C.MOVING)):
        assert re.search(rf"#define UAVQP_SEPARATION_{name} {val}\b", h), name
    body = re.search(r"typedef struct uavqp_separation_params \{(.*?)\} uavqp_separation_params;", h, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+(\w+);", body, re.M)
    from uav_motion_planning_amd import _lib
    assert [(n, {"int32_t": ctypes.c_int32, "double": ctypes.c_double}[t]) for t, n in fields] == list(_lib.SeparationParams._fields_)
    assert (_lib.UAVQP_SEPARATION_CERTIFIED, _lib.UAVQP_SEPARATION_VIOLATED, _lib.UAVQP_SEPARATION_MOVING) == (C.CERTIFIED, C.VIOLATED, C.MOVING)
    assert C.MAX_VEHICLES == _lib.UAVQP_SWARM_MAX_VEHICLES
    for name in names:
        assert name in _lib.SYMBOLS


def test_out_of_scope_and_the_pointer_from_the_swarm_optimiser():
    h = header()
    own = h[h.index("/* Certified continuous-time separation"):h.index("typedef struct uavqp_separation_params")]
    for phrase in ("merged knots", "squared-distance polynomial", "adaptive subdivision", "non-cooperative obstacles", "uavqp_swarm_optimize_"):
        assert phrase in own[own.index("Out of scope"):], phrase
    opt = h[h.index("/* Swarm optimiser"):h.index("typedef struct uavqp_swarm_opt_params")]
    assert "separation is reported by d_min_sep_out on the swarm's clock samples only" in opt      # (the sentence is extended, not replaced)
    assert "uavqp_separation_certificate_" in opt
    with open(os.path.join(ROOT, "uav_motion_planning_amd", "csrc", "qp_separation_cert.h")) as fh:
        k = fh.read()
    assert "merged knots" in k[k.index("Out of scope"):]


def test_default_params_without_a_device():
    from uav_motion_planning_amd import _lib
    sp = _lib.SeparationParams()
    _lib.lib().uavqp_default_separation_params(ctypes.byref(sp))
    assert (sp.struct_size, sp.depth, sp.n_cells, sp.clock_start, sp.dt, sp.downwash, sp.d_req) == (ctypes.sizeof(_lib.SeparationParams), 2, 64, 0.0, 0.1, 1.0, 1.0)
    assert sp.struct_size == 48
    assert {k: getattr(sp, k) for k in C.DEFAULTS} == C.DEFAULTS
    assert len(_lib.lib().uavqp_separation_certificate_device.argtypes) == len(_lib.lib().uavqp_separation_certificate_host.argtypes) == 17
