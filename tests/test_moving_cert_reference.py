"""CPU: the method of uavqp_moving_certificate_* (include/uavqp.h, csrc/qp_moving_cert.h) as tests/moving_cert_reference.py restates it,
against the mpmath truth of the certified curves, and the conditions the inputs of tests/test_gpu_moving_cert.py must meet, asserted here
on the exact solve before a GPU is involved.

Soundness has NO tolerance: lower <= truth at 64 instants of every depth-3 leaf (per certificate leaf, its ends included) and
truth(witness) <= upper, compared in mpmath.  Everything that compares two evaluations of the method (formation, radius, nesting) uses the
allowance of the deciding pair, sqrt(3) max Gs + R, which the reference returns."""
import ctypes
import os
import re

import numpy as np
import pytest

import moving_cert_reference as R
import moving_penalty_reference as MP
import test_moving_penalty_reference as C
from uav_motion_planning_amd import _lib

# the reference below restates THIS entry of the library: without its binding there is nothing to restate
PARAMS, ENTRIES = _lib.MovingCertParams, [n for n in _lib.SYMBOLS if "moving_cert" in n]
assert len(ENTRIES) == 3, ENTRIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_MS = (2, 1, 3)
SMALL_SETS = (6, 1, 3)      # all six kinds of track on trajectory 0


def small(oracle, r):
    b = MP.batch(r, SMALL_MS, 70 + r)
    obs = R.obstacles_for(b, C.exact_solver(oracle), 80 + r, SMALL_SETS, close=(1,))
    return b, C.solved(oracle, b), obs


_truths = {}


def truth_of(oracle, r, downwash):
    if (r, downwash) not in _truths:
        b, c, obs = small(oracle, r)
        _truths[(r, downwash)] = R.truth(r, b["seg_offsets"], b["times"], c, obs, downwash=downwash)
    return _truths[(r, downwash)]


def test_params_struct_matches_the_header_and_the_defaults():
    src = open(os.path.join(ROOT, "include", "uavqp.h")).read()
    body = re.search(r"typedef struct uavqp_moving_cert_params \{(.*?)\} uavqp_moving_cert_params;", src, flags=re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+([a-z_]+);", body, flags=re.M)
    ctype = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.MovingCertParams._fields_)
    assert re.search(r"#define UAVQP_MOVING_CERT_CERTIFIED 1\b", src) and re.search(r"#define UAVQP_MOVING_CERT_VIOLATED 2\b", src)
    assert (_lib.UAVQP_MOVING_CERT_CERTIFIED, _lib.UAVQP_MOVING_CERT_VIOLATED) == (R.CERTIFIED, R.VIOLATED) == (1, 2)
    p = _lib.MovingCertParams()
    _lib.lib().uavqp_default_moving_cert_params(ctypes.byref(p))      # (callable without a device)
    assert p.struct_size == ctypes.sizeof(_lib.MovingCertParams)
    assert (p.depth, p.downwash, p.d_req) == (R.DEFAULTS["depth"], R.DEFAULTS["downwash"], R.DEFAULTS["d_req"]) == (3, 1.0, 1.0)
    # the notes that said there is no such certificate are gone
    assert "no certificate of its own yet" not in src and "a certificate of its own" not in src and "concatenates a vehicle" not in src


@pytest.mark.parametrize("downwash", [1.0, 1.5])
@pytest.mark.parametrize("r", [3, 4])
def test_lower_and_upper_are_sound_against_the_truth(oracle, r, downwash):
    b, c, obs = small(oracle, r)
    tracks = MP.obstacle_tracks(r, obs)
    assert {len(t[1]) for t in tracks} >= {1, 5} and set(obs["radius"]) == {0.0, 0.3}
    line = tracks[1]      # kind "line": a constant-velocity prediction
    assert len(line[1]) == 1 and not line[2][:, :, 2:].any() and line[2][:, :, 1].any()
    tr = truth_of(oracle, r, downwash)
    for depth in (0, 2, 5):
        ref = R.certificate(r, b["seg_offsets"], b["times"], c, obs, depth=depth, downwash=downwash, d_req=0.8)
        # (at depth 0 a leaf is a whole segment: with durations that are no dyadic numbers its rounded end is not trusted, and it lies in
        #  ONE obstacle piece only where that piece is longer than the segment)
        assert ref["states"] >= {R.WAITING, R.ARRIVED, R.STRADDLING} and (depth == 0 or R.MOVING in ref["states"]), ref["states"]
        assert ref["whole_wait"], "no obstacle waits for the whole flight"
        assert np.all(np.isfinite(ref["gap"]))
        bad = R.soundness_failures(ref, tr, depth, tag=f"r={r} downwash={downwash} depth={depth}")
        assert not bad, "\n".join(bad[:10])
        width = ref["gap"][:, 1] - ref["gap"][:, 0]
        print(f"r={r} downwash={downwash} depth={depth}: upper - lower median {np.median(width):.3f} m, largest {width.max():.3f} m; "
              + ", ".join(f"{k} {int(np.sum([R.state(w) == k for w in ref['seg_verdict']]))}" for k in ("certified", "violated", "undecided")))
        assert np.all(width >= 0.0)


def short_piece_case(r, jump):
    """a trajectory of ONE segment, T = 1 s, against a constant-velocity obstacle cut into 24 pieces of 0.05 s (jump: the pieces from the
    tenth on are moved by 0.5 m)"""
    Ct = np.zeros((3, 1, 2 * r))
    Ct[:, 0, 0] = (0.0, 0.0, 1.0)
    Ct[:, 0, 1] = (2.0, 0.3, 0.0)
    Ct[:, 0, 3] = (-0.8, 0.5, 0.1)
    p0, v = np.array([0.4, 1.1, 1.2]), np.array([1.5, -0.9, 0.1])
    Co = np.zeros((3, 24, 2 * r))
    for k in range(24):
        Co[:, k, 0] = p0 + v * (0.05 * k) + (np.array([0.0, 0.5, 0.0]) if jump and k >= 10 else 0.0)
        Co[:, k, 1] = v
    return R.single_case(r, [1.0], Ct, [(np.full(24, 0.05), Co, -0.1, 0.3 if jump else 0.0)])


@pytest.mark.parametrize("jump", [False, True], ids=["continuous", "jump_at_a_knot"])
@pytest.mark.parametrize("r", [3, 4])
def test_a_leaf_that_straddles_many_short_pieces(r, jump):
    so, T, c, obs = short_piece_case(r, jump)
    tr = R.truth(r, so, T, c, obs)
    for depth in (0, 3):
        ref = R.certificate(r, so, T, c, obs, depth=depth, d_req=0.5)
        if depth == 0:
            assert ref["states"] == {R.STRADDLING}
        bad = R.soundness_failures(ref, tr, depth, tag=f"short pieces r={r} depth={depth}")
        assert not bad, "\n".join(bad[:10])
    if jump:      # both values at the knot belong to the curve: the truth there is the smaller gap
        inst, _ = tr
        assert float(min(inst[0])) < float(ref["gap"][0, 1])


@pytest.mark.parametrize("r", [3, 4])
def test_formation_is_certified_by_the_polynomial_difference_not_by_boxes(oracle, r):
    so, T, c, obs = R.formation_case(r, C.exact_solver(oracle))
    ref = R.certificate(r, so, T, c, obs, depth=0, d_req=1.2)
    # (the allowance is added to 1.25 in float64: the comparison itself loses up to an ulp of 1.25 per operation)
    assert np.all(np.abs(ref["gap"] - 1.25) <= ref["allow"] + 4.0 * np.spacing(1.25)), ref["gap"]
    assert np.all(ref["seg_verdict"] == R.CERTIFIED) and ref["verdict"][0] == R.CERTIFIED and ref["states"] == {R.MOVING}
    box = R.certificate(r, so, T, c, obs, depth=0, d_req=1.2, force_box=True)
    assert not np.any(box["seg_verdict"] & R.CERTIFIED) and np.all(box["gap"][:, 0] < 1.2)


@pytest.mark.parametrize("r", [3, 4])
def test_head_on_pass_between_two_samples(r):
    import mpmath
    so, T, c, obs = R.head_on(r)
    d_req = 0.5
    sampled = MP.penalty(r, so, T, c, obs, grads=False, samples_per_seg=8)["min_gap"][0]
    assert sampled > d_req and abs(sampled - 0.656) < 1e-3
    tr = R.truth(r, so, T, c, obs)
    at36 = tr[1](0, 0, 36, 64)      # the closest approach, 0.5625 s
    assert abs(float(at36) - 0.2) < 1e-12 and float(min(tr[0][0])) >= 0.2 - 1e-12
    d3 = R.certificate(r, so, T, c, obs, depth=3, d_req=d_req)
    assert R.state(d3["verdict"][0]) in ("undecided", "violated") and not d3["seg_verdict"][0] & R.CERTIFIED
    assert abs(d3["gap"][0, 1] - sampled) <= d3["allow"][0, 1] + 1e-9 * sampled      # the witnesses of depth 3 ARE the eight samples
    d6 = R.certificate(r, so, T, c, obs, depth=6, d_req=d_req)
    assert R.state(d6["verdict"][0]) == "violated" and abs(d6["gap"][0, 1] - 0.2) <= 0.05 and d6["where"][0, 3] == 36
    for ref, depth in ((d3, 3), (d6, 6)):
        assert not R.soundness_failures(ref, tr, depth)
        assert mpmath.mpf(float(ref["gap"][0, 0])) <= at36 <= mpmath.mpf(float(ref["gap"][0, 1]))
    print(f"r={r}: sampled gap {sampled:.3f} m; depth 3 [{d3['gap'][0, 0]:.3f}, {d3['gap'][0, 1]:.3f}] {R.state(d3['verdict'][0])}; "
          f"depth 6 [{d6['gap'][0, 0]:.3f}, {d6['gap'][0, 1]:.3f}] {R.state(d6['verdict'][0])}; true minimum {float(at36):.3f} m")


@pytest.mark.parametrize("r", [3, 4])
def test_a_larger_radius_lowers_the_bounds_it_decides(oracle, r):
    b, c, obs = small(oracle, r)
    base = R.certificate(r, b["seg_offsets"], b["times"], c, obs, depth=2, d_req=0.8)
    deciding = np.concatenate([base["where"][:, 0], base["where"][:, 2]])
    o = int(np.bincount(deciding[deciding >= 0]).argmax())      # the obstacle that decides the most bounds
    more = dict(obs, radius=obs["radius"] + 0.3 * (np.arange(obs["radius"].size) == o))
    got = R.certificate(r, b["seg_offsets"], b["times"], c, more, depth=2, d_req=0.8)
    n = 0
    for col, which in ((0, 0), (1, 2)):
        decided = base["where"][:, which] == o
        assert np.all(got["where"][decided, which] == o)
        n += int(decided.sum())
        assert np.all(np.abs(got["gap"][decided, col] - (base["gap"][decided, col] - 0.3)) <= base["allow"][decided, col] + got["allow"][decided, col])
        assert np.all(got["gap"][:, col] <= base["gap"][:, col])
    assert n >= 2


@pytest.mark.parametrize("r", [3, 4])
def test_bounds_nest_from_one_depth_to_the_next(oracle, r):
    b, c, obs = small(oracle, r)
    prev = R.certificate(r, b["seg_offsets"], b["times"], c, obs, depth=0, downwash=1.5)
    for depth in range(1, 6):
        cur = R.certificate(r, b["seg_offsets"], b["times"], c, obs, depth=depth, downwash=1.5)
        slack = prev["allow"] + cur["allow"]
        assert np.all(cur["gap"][:, 0] >= prev["gap"][:, 0] - slack[:, 0]), depth
        assert np.all(cur["gap"][:, 1] <= prev["gap"][:, 1] + slack[:, 1]), depth
        prev = cur


def test_special_cases_of_the_reference(oracle):
    r = 3
    b, c, obs = small(oracle, r)
    so = b["seg_offsets"]
    status = np.array([1, 0, 1], dtype=np.int32)
    none = dict(obs, traj_set=np.array([0, 1, -1], dtype=np.int32))
    ref = R.certificate(r, so, b["times"], c, none, status=status, d_req=0.8)
    s1, s2 = slice(int(so[1]), int(so[2])), slice(int(so[2]), int(so[3]))
    assert np.all(ref["gap"][s1] == np.inf) and np.all(ref["seg_verdict"][s1] == 0) and ref["verdict"][1] == 0      # not solved
    assert np.all(ref["gap"][s2] == np.inf) and np.all(ref["seg_verdict"][s2] == R.CERTIFIED) and ref["verdict"][2] == R.CERTIFIED
    assert np.all(ref["where"][int(so[1]):] == R.NONE) and np.all(ref["peak"][1:] == np.inf)
    broken = c.copy()
    broken[3] = np.nan      # segment 0 of trajectory 0, axis x
    ref = R.certificate(r, so, b["times"], broken, obs, d_req=0.8)
    assert np.all(np.isnan(ref["gap"][0])) and np.all(ref["where"][0] == R.NONE) and ref["seg_verdict"][0] == 0
    assert np.all(np.isfinite(ref["gap"][1:])) and np.all(np.isnan(ref["peak"][0])) and ref["verdict"][0] == 0 and np.all(np.isfinite(ref["peak"][1:]))


@pytest.mark.parametrize("near_after", [False, True], ids=["near_before_the_knot", "near_after_the_knot"])
@pytest.mark.parametrize("r", [3, 4])
def test_a_rounded_leaf_end_beside_a_knot_with_a_jump(r, near_after):
    """ONE segment whose arrival S + T is not a double: tb = fl(S + T).  The obstacle jumps by 1.7 m at a knot that IS that double, so the
    real end of the leaf lies on one side of the knot and the rounded one on it -- on which side depends on the rounding.  lower must hold
    at the real last instant whichever piece it is in, and no witness is taken there."""
    from fractions import Fraction
    sides = set()
    for S, T0 in R.ROUNDED_ENDS:
        so, T, c, obs, K1, real = R.rounded_end_case(r, S, T0, near_after)
        if real == Fraction(K1):
            continue
        sides.add(real > Fraction(K1))
        y = (2.0, 0.3) if near_after else (0.3, 2.0)
        assert R.SC.knots([K1, 0.6], 0.0)[1] == K1
        tr = R.truth(r, so, T, c, obs)
        last = float(tr[0][0][-1])      # the truth at the real arrival: the piece it really lies in
        assert abs(last - (y[1] if real > Fraction(K1) else y[0])) < 0.3
        for depth in (0, 3):
            ref = R.certificate(r, so, T, c, obs, depth=depth, d_req=0.5)
            bad = R.soundness_failures(ref, tr, depth, tag=f"S={S} T={T0} depth={depth}")
            assert not bad, "\n".join(bad[:5])
            assert ref["where"][0, 3] < (1 << depth), "the open right end gave a witness"
    assert sides == {False, True}, "both rounding directions must occur"


def test_a_nan_duration_spoils_its_segment_and_every_later_one(oracle):
    r = 3
    b, c, obs = small(oracle, r)
    so = b["seg_offsets"]
    T = b["times"].copy()
    t = 2      # three segments
    T[int(so[t]) + 1] = np.nan
    ref = R.certificate(r, so, T, c, obs, d_req=0.8)
    s0 = int(so[t])
    assert np.all(np.isfinite(ref["gap"][:s0 + 1])) and np.all(np.isnan(ref["gap"][s0 + 1:s0 + 3])) and np.all(ref["where"][s0 + 1:s0 + 3] == R.NONE)
    assert not ref["seg_verdict"][s0 + 1:s0 + 3].any() and np.all(np.isnan(ref["peak"][t])) and ref["verdict"][t] == 0
    T[int(so[t]) + 1] = -0.5      # a duration <= 0 spoils its own segment alone: the clock goes on
    ref = R.certificate(r, so, T, c, obs, d_req=0.8)
    assert np.all(np.isnan(ref["gap"][s0 + 1])) and np.all(np.isfinite(ref["gap"][[s0, s0 + 2]]))


@pytest.mark.parametrize("name", list(R.gpu_cases()))
def test_the_gpu_inputs_meet_their_conditions(oracle, name):
    """d_req lies more than two allowances from every bound, and at most 10 % of the segments have a runner-up within two allowances of
    the winner (those are left out of the comparison of `where`)"""
    b = R.gpu_batch(name)
    obs = R.gpu_obstacles(name, C.exact_solver(oracle))
    c = C.solved(oracle, b)
    seen = set()
    for depth in R.GPU_DEPTHS:
        ref = R.certificate(b["r"], b["seg_offsets"], b["times"], c, obs, depth=depth, downwash=1.5, d_req=R.GPU_D_REQ)
        assert R.two_allowances_away(ref, R.GPU_D_REQ)
        assert R.tie_fraction(ref) <= 0.10, (name, depth, R.tie_fraction(ref))
        assert ref["allow"].max() < 1e-9
        seen |= {R.state(w) for w in ref["seg_verdict"][np.isfinite(ref["gap"][:, 0])]}
    assert seen & {"certified", "violated"}, seen
