"""CPU contract of the sampler tests: the inputs of tests/test_gpu_samplers.py are what they were designed to be, their time grids are
exact (no sample can change class through a fused multiply-add: nothing is skipped), the decisive obstacle points have their margins,
and the derived tolerance 32 * 2^-53 * S bounds a float64 Horner evaluation with a factor ten to spare.

The reference (tests/sampler_reference.py) restates include/uavqp.h: the segment rule in float64 exactly as stated, everything else in
np.longdouble."""
import numpy as np
import pytest

import sampler_reference as R

LD = R.LD


def _all_eval_grids():
    for r in (3, 4):
        for name, case in R.eval_cases(r).items():
            for g in case["grids"]:
                yield r, name, case, g


def test_the_vectorised_rule_is_the_scalar_rule_of_the_header():
    n = 0
    for r, name, case, g in _all_eval_grids():
        ref, so = g["ref"], case["seg_offsets64"]
        step = 1 if g["kind"] != "coarse" else 5
        for b in range(case["n_traj"]):
            T = case["times"][so[b]:so[b + 1]]
            if T.size == 0:
                assert not ref["out"][b].any() and not ref["S"][b].any()
                continue
            for s in range(0, g["n_samples"], step):
                idx, tl, cl = R.segment_rule_scalar(T, ref["t"][s])
                assert (idx, tl, cl) == (ref["idx"][b, s], ref["tl"][b, s], ref["clamped"][b, s]), (r, name, g["name"], b, s)
                n += 1
    assert n > 5000


def test_every_designed_time_grid_is_exact():
    """t0 + s * dt and every running t - T_i, rounded once from longdouble, are the float64 values bit for bit: the share of samples
    that would have to be skipped for closeness to a boundary is zero, as a condition."""
    skipped = total = 0
    for r, name, case, g in _all_eval_grids():
        skipped += int((~g["ref"]["exact"]).sum())
        total += g["ref"]["exact"].size
        assert g["dt"] >= 2.0 ** -14 and np.all(case["times"] * 64 == np.round(case["times"] * 64))
    for r in (3, 4):
        for case in list(R.ellipsoid_cases(r).values()) + [R.endpoint_case(r), R.endpoint_lane0_case(r), R.degenerate_case(r)] + list(R.grid_geometry_cases(r).values()) + list(R.knot_cases(r).values()):
            skipped += int((~case["ref"]["exact"]).sum())
            total += case["ref"]["exact"].size
    assert skipped == 0 and total > 20000


@pytest.mark.parametrize("r", [3, 4])
def test_each_designed_sample_is_in_the_class_it_was_designed_for(r):
    seen = set()
    for name, case in R.eval_cases(r).items():
        so = case["seg_offsets64"]
        assert np.unique(case["coeff"]).size == case["coeff"].size                 # every (trajectory, axis, segment, power) distinct
        for g in case["grids"]:
            ref = g["ref"]
            if g["kind"] == "coarse":
                for b in range(case["n_traj"]):
                    T = case["times"][so[b]:so[b + 1]]
                    if T.size == 0:
                        continue
                    c = R.sample_classes(T, ref["t"], ref["idx"][b], ref["tl"][b], ref["clamped"][b])
                    assert c["negative"][:8].all() and np.all(ref["idx"][b][:8] == 0) and np.all(ref["tl"][b][:8] < 0)      # t < 0: segment 0, extrapolated
                    assert c["clamped"][-100:].all() and set(ref["idx"][b]) == set(range(T.size))                         # far past the end; every segment visited
                    seen.add("negative"), seen.add("far_past_end")
                continue
            b, k = g["b"], g["k"]
            T = case["times"][so[b]:so[b + 1]]
            M, last = T.size, g["k"] == T.size - 1
            c = R.sample_classes(T, ref["t"], ref["idx"][b], ref["tl"][b], ref["clamped"][b])
            where = "last" if last else ("first" if k == 0 else "interior")
            if g["kind"] == "window":
                assert g["t0"] != 0.0
                assert np.all(ref["idx"][b][:10] == k) and not ref["clamped"][b][:10].any()
                assert c["on_knot"][8] and ref["tl"][b][8] == T[k]                                         # exactly on the knot: the earlier segment
                assert c["in_slack"][9] and ref["tl"][b][9] == T[k] + 2.0 ** -14                            # 6.1e-5 beyond: still the earlier one, past its end
                if last:
                    assert ref["clamped"][b][10:].all() and np.all(ref["tl"][b][10:] == T[k]) and np.all(ref["idx"][b][10:] == k)
                else:
                    assert np.all(ref["idx"][b][10:] == k + 1) and ref["tl"][b][10] == 2.0 ** -13 and not ref["clamped"][b][10:].any()
                seen |= {("on_knot", where), ("in_slack", where), ("clamped" if last else "advanced", where)}
            elif g["kind"] == "stay":
                assert ref["idx"][b][0] == k and not ref["clamped"][b][0] and ref["tl"][b][0] <= np.float64(T[k] + 1e-4)
                if k == 0:
                    assert g["t0"] == float(np.float64(T[0] + 1e-4))                                        # fl(T_0 + 1e-4) itself
                    seen.add(("threshold_itself", "clamp" if last else "advance"))
                seen.add(("stay", where))
            else:
                assert g["t0"] == np.nextafter(next(x for x in case["grids"] if x["name"] == g["name"].replace("leave", "stay"))["t0"], np.inf)
                assert ref["clamped"][b][0] if last else (ref["idx"][b][0] == k + 1 and not ref["clamped"][b][0])
                seen.add(("leave", where))
        assert (case["M"] == 1).any() or name == "uniform17"
    assert tuple(R.eval_cases(r)["ragged"]["M"]) == R.RAGGED_MS and R.eval_cases(r)["uniform17"]["uniform"] == 17
    assert R.RAGGED_MS[3] == 0 and R.RAGGED_MS.count(1) == 2 and 17 in R.RAGGED_MS
    want = {"negative", "far_past_end", ("threshold_itself", "advance"), ("threshold_itself", "clamp")}
    for where in ("first", "interior", "last"):
        want |= {("on_knot", where), ("in_slack", where), ("stay", where), ("leave", where), ("clamped" if where == "last" else "advanced", where)}
    assert want <= seen, want - seen


@pytest.mark.parametrize("r", [3, 4])
def test_neighbouring_segments_are_discontinuous_in_value_and_every_derivative(r):
    for name, case in R.eval_cases(r).items():
        so = case["seg_offsets64"]
        for b in range(case["n_traj"]):
            T = case["times"][so[b]:so[b + 1]]
            if T.size < 2:
                continue
            C = R.traj_coeff(r, so, case["coeff"], b)
            i = np.arange(T.size - 1)
            end, _ = R.poly_longdouble(C, i, T[:-1])
            start, _ = R.poly_longdouble(C, i + 1, np.zeros(T.size - 1))
            gap = np.max(np.abs(end - start), axis=2)                     # per knot and derivative order, the largest jump over the axes
            assert float(gap.min()) > 0.05, (name, b, float(gap.min()))


def test_float64_horner_stays_ten_times_below_the_derived_tolerance():
    """|Horner in float64 - longdouble| <= 0.1 * 32 * 2^-53 * S on every designed sample and derivative order."""
    worst = 0.0
    for r, name, case, g in _all_eval_grids():
        ref, so = g["ref"], case["seg_offsets64"]
        for b in range(case["n_traj"]):
            if so[b + 1] == so[b]:
                continue
            h = R.horner_float64(R.traj_coeff(r, so, case["coeff"], b), ref["idx"][b], ref["tl"][b])
            ratio = np.abs(LD(1) * h - ref["out"][b]) / (LD(32 * R.U53) * ref["S"][b])
            worst = max(worst, float(ratio.max()))
    print(f"float64 Horner against longdouble: at most {worst:.3f} of 32 * 2^-53 * S")
    assert worst < 0.1


# ---------------------------------------------------------------------------------------------------------------------------------
# length
# ---------------------------------------------------------------------------------------------------------------------------------
def test_length_inputs_and_the_accumulated_count():
    for r in (3, 4):
        cases = R.length_cases(r)
        # dt = 2^-6: 1 sample (dt exceeds the total time), 2, 64, 65, 129; a zero-segment trajectory in the middle: 0 samples, length 0, mean NaN
        for name in ("dyadic", "line"):
            ref = cases[name]["ref"]
            assert list(ref["n"]) == [1, 2, 64, 0, 65, 129, 32]
            assert ref["length"][0] == 0 and ref["length"][3] == 0 and np.isnan(ref["mean"][3]) and ref["mean"][0] == 0
            assert np.all(ref["bound"][[1, 2, 4, 5, 6]] < 1e-11 * ref["length"][[1, 2, 4, 5, 6]])
        # a straight line: the closed form |v| (n - 1) dt
        line = cases["line"]
        speed = np.sqrt(np.sum((LD(1) * line["v"]) ** 2, axis=1))
        want = speed * (np.maximum(line["ref"]["n"], 1) - 1) * LD(R.LENGTH_DT)
        want[3] = 0
        assert np.all(np.abs(line["ref"]["length"] - want) <= line["ref"]["bound"] + LD(1e-300))
        # the reference's own grid: dt = 0.01, 1.0 s per segment.  After 100 M additions the accumulated t is >= M for M = 1, 2 (100 M
        # samples) and still below M for M = 3 .. 7 (one sample more): both outcomes
        # the kernel's own copy of the segment rule: samples on the knot, inside the slack and exactly on the threshold
        sl, th = cases["slack"], cases["threshold"]
        idx, tl, _, ex = R.segment_rule(sl["times"], np.arange(768) * sl["dt"])
        assert sl["ref"]["n"][0] == 768 and ex.all() and list(idx[511:515]) == [0, 0, 0, 1] and tl[512] == sl["times"][0] and tl[513] > sl["times"][0]
        assert th["ref"]["n"][0] == 2 and th["dt"] == float(np.float64(0.5 + 1e-4)) and R.segment_rule_scalar(th["times"], th["dt"])[0] == 0
        assert R.segment_rule_scalar(th["times"], np.nextafter(th["dt"], np.inf))[0] == 1
        acc = cases["accumulated"]
        assert list(acc["ref"]["n"]) == [100, 200, 301, 401, 501, 601, 701]
    n1, t1 = R.count_samples(1.0, 0.01)
    n3, t3 = R.count_samples(3.0, 0.01)
    assert (n1, n3) == (100, 301) and t1 >= 1.0 and t3 > 3.0
    t = np.float64(0.0)
    for _ in range(300):
        t = np.float64(t + np.float64(0.01))
    assert t < 3.0                                   # 300 additions end BELOW 3.0: sample 300 exists
    t = np.float64(0.0)
    for _ in range(100):
        t = np.float64(t + np.float64(0.01))
    assert t >= 1.0                                  # 100 additions end at or above 1.0: sample 100 does not
    # the samples s * 0.01 are not dyadic, but none comes closer than 1e-5 to a threshold T_i + 1e-4 (knots at whole seconds)
    ts = np.arange(701) * 0.01
    frac = ts - np.round(ts)
    assert np.min(np.abs(frac - 1e-4)) > 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# ellipsoid
# ---------------------------------------------------------------------------------------------------------------------------------
def _pair_margins(case):
    """(margins of the planted pairs, margins of all other candidate-or-not pairs, distances to the candidate sphere of the planted pairs)."""
    ref = case["ref"]
    planted, others, sphere = [], [], []
    live = [b for b in range(case["n_traj"]) if case["seg_offsets64"][b + 1] > case["seg_offsets64"][b]]
    for b, (m, dsph, inv) in zip(live, ref["margins"]):
        mask = np.zeros(m.shape, dtype=bool)
        for (pb, s, _, _), slot in zip(case.get("plants", []), case.get("slots", [])):
            if pb == b:
                mask[inv[s], slot] = True
                sphere.append(dsph[inv[s], slot])
        planted.append(m[mask]), others.append(m[~mask])
    return np.concatenate(planted), np.concatenate(others), np.array(sphere, dtype=LD)


@pytest.mark.parametrize("r", [3, 4])
def test_decisive_obstacle_points_have_margin(r):
    for name, case in R.ellipsoid_cases(r).items():
        planted, others, sphere = _pair_margins(case)
        assert planted.size == len(case["plants"]) and float(planted.min()) >= 1e-7 and float(planted.max()) <= 2e-6, (name, planted)
        assert float(np.nanmin(others)) >= 1e-3, (name, float(np.nanmin(others)))
        assert float(sphere.min()) >= 1e-6, name
        for (b, s, _, inside) in case["plants"]:
            if inside:
                assert case["ref"]["flags"][b, s] == 1, (name, b, s)
    geo = R.grid_geometry_cases(r)
    for case in [R.endpoint_case(r), R.endpoint_lane0_case(r), R.degenerate_case(r), geo["neighbours"], geo["bbox"]] + list(R.knot_cases(r).values()):
        _, others, _ = _pair_margins(dict(case, plants=[], slots=[]))
        assert float(others[np.isfinite(others)].min()) >= 1e-3            # (NaN: the degenerate attitudes)
    for name in ("pooled", "pooled_miss"):
        _, others, _ = _pair_margins(dict(R.grid_geometry_cases(r)[name], plants=[], slots=[]))
        s = np.sort(others[np.isfinite(others)])
        assert 1e-7 <= float(s[0]) <= 2e-6 and float(s[1]) >= 1e-3


@pytest.mark.parametrize("r", [3, 4])
def test_ellipsoid_inputs_tell_wrong_models_apart(r):
    """The designed verdicts change when the thin and the wide axes are swapped, when gravity is left out of the attitude, and when every
    attitude is taken for hover: a kernel with one of these faults cannot pass."""
    case = R.ellipsoid_cases(r)["directions"]
    args = (r, case["n_traj"], case["uniform"], case["seg_offsets64"], case["times"], case["coeff"], case["n_samples"], case["t0"], case["dt"], case["obs"])
    good = case["ref"]["flags"]
    assert R.ROBOT_H != R.ROBOT_R
    assert not np.array_equal(R.ellipsoid_reference(*args, swap_axes=True)["flags"], good)
    assert not np.array_equal(R.ellipsoid_reference(*args, gravity=0.0)["flags"], good)
    assert not np.array_equal(R.ellipsoid_reference(*args, gravity=1e9)["flags"], good)             # (acc negligible against it: hover)
    # the planted points: inside ones collide, outside ones do not, on every attitude and body direction
    seen = set()
    for (b, s, u, inside) in case["plants"]:
        assert bool(good[b, s]) == inside
        seen.add((u, case["ref"]["clamped"][b, s]))
    assert {u for u, _ in seen} == set(R.BODY_DIRS)
    assert good[0, 0] == 1 and good[3, case["n_samples"] - 1] == 1 and case["ref"]["first_hit"][0] == 0
    assert sorted(case["slots"])[:1] == [0] and {1023, 1024, 2499} <= set(case["slots"]) and case["obs"].shape[0] == 2500


@pytest.mark.parametrize("r", [3, 4])
def test_ellipsoid_cases_hold_the_designed_situations(r):
    cases = R.ellipsoid_cases(r)
    for n_obs in (1, 1024, 1025):
        c = cases[f"tile{n_obs}"]
        assert c["obs"].shape[0] == n_obs and c["slots"] == [n_obs - 1] and list(c["ref"]["first_hit"]) == [12, 5]
    rg = cases["ragged"]
    assert rg["M"][2] == 0 and rg["ref"]["first_hit"][2] == rg["n_samples"] and not rg["ref"]["flags"][2].any()          # zero segments: collision-free
    assert rg["ref"]["first_hit"][0] == rg["n_samples"]                                                                  # nothing near trajectory 0
    f4 = rg["ref"]["flags"][4]
    assert f4.any() and np.array_equal(f4.astype(bool), rg["ref"]["clamped"][4])                                          # collides only past the end
    bl = cases["blocks"]
    assert bl["n_samples"] > 512 and list(bl["ref"]["first_hit"]) == [300, 259]
    assert bl["ref"]["flags"][0, 300] and bl["ref"]["flags"][0, 301] and bl["ref"]["flags"][0, 520] and not bl["ref"]["flags"][1, 258]
    ep = R.endpoint_case(r)
    assert list(ep["ref"]["first_hit"]) == [0, 31, 1]
    assert np.array_equal(ep["ref"]["flags"].astype(bool), ep["ref"]["clamped"])                                         # only the end point collides
    lanes = (np.arange(3)[:, None] * 32 + np.arange(32)[None, :]) % 64
    assert [int(lanes[b, ep["ref"]["first_hit"][b]]) for b in range(3)] == [0, 63, 1]
    kn = R.knot_cases(r)
    assert list(kn["knot_window"]["ref"]["flags"][0]) == [1] * 10 + [0] * 22           # on the knot (8) and inside the slack (9): the first segment
    assert kn["knot_threshold"]["t0"] == float(np.float64(kn["knot_threshold"]["times"][0] + 1e-4))
    assert list(kn["knot_threshold"]["ref"]["first_hit"]) == [0] and list(kn["knot_above"]["ref"]["first_hit"]) == [1]
    e0 = R.endpoint_lane0_case(r)
    assert list(e0["ref"]["first_hit"]) == [48, 16] and (48 + 16) % 64 == 0 and not e0["ref"]["clamped"][0].any()        # lane 0 with s > 0
    assert np.array_equal(e0["ref"]["flags"].astype(bool), e0["ref"]["clamped"]) and not e0["ref"]["clamped"][1, 15]
    by = R.beyond_grid_case(r, 256)                                                      # an MI355X has 256 compute units
    ns, ref = by["n_samples"], by["ref"]
    assert 2 * ns > 256 * 16 * 256 and 2 * ns > 64 * 64 * 256 and ref["exact"].all()
    assert ref["first_hit"][1] == 5 and ref["flags"][1].sum() == 1
    assert np.array_equal(ref["flags"][0].astype(bool), ref["clamped"][0]) and 0 < ref["first_hit"][0] < 20
    planted, others, sphere = _pair_margins(by)
    assert 1e-7 <= float(planted.min()) <= 2e-6 and float(others.min()) >= 1e-3 and float(sphere.min()) >= 1e-6
    dg = R.degenerate_case(r)
    # no thrust and b3 parallel to x: collision-free although a point sits ON the sample; a hair off the degenerate direction: collides
    assert list(dg["ref"]["first_hit"]) == [1, 1, 0]


def test_degenerate_attitudes_follow_the_oracle(oracle):
    """oracle/ellipsoid.c (the project's restatement of KinoAstar::isCollisionFree) divides by the zero norm: NaN axes, |E^-1 d| <= 1 is
    false, the sample is collision-free.  The reference module's rule is that one."""
    dg = R.degenerate_case(3)
    acc = ((0.0, 0.0, -R.G), (3.0, 0.0, -R.G), (3.0, 1e-3, -R.G))
    for b in range(3):
        free = oracle.is_collision_free(dg["obs"][b], np.array(acc[b]), dg["obs"], R.ROBOT_R, R.ROBOT_H)
        assert free == (dg["ref"]["first_hit"][b] == 1), b


def test_grid_geometry_is_what_it_was_designed_to_be():
    g = R.grid_geometry_cases(3)
    nb = g["neighbours"]
    org, cell = nb["obs"].min(axis=0), 0.5
    assert np.array_equal(org, [-4.0, -4.0, -4.0]) and nb["n_traj"] == 26 and list(nb["ref"]["first_hit"]) == [0] * 26
    pos = np.array([p[0] for p in nb["ref"]["pos"]], dtype=np.float64)
    d_cell = np.floor((nb["obs"][2:] - org) / cell).astype(int) - np.floor((pos - org) / cell).astype(int)
    assert sorted(map(tuple, d_cell)) == sorted((dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0))
    # every sample collides with ITS point only
    for k in range(26):
        m = nb["ref"]["margins"][k][0][0]
        assert np.flatnonzero(m + 1 <= 2)[0] == 2 + k and np.count_nonzero(m + 1 <= 2) == 1 and np.isfinite(m).all()
    assert list(g["bbox"]["ref"]["first_hit"]) == [0, 1, 0, 1, 0, 1]
    lo, hi = g["bbox"]["obs"].min(axis=0), g["bbox"]["obs"].max(axis=0)
    p = np.array([q[0] for q in g["bbox"]["ref"]["pos"]], dtype=np.float64)
    assert np.all((p < lo).any(axis=1) | (p > hi).any(axis=1))                                      # all six outside the bounding box
    for name, want in (("pooled", 0), ("pooled_miss", 1)):
        c = g[name]
        fh = c["ref"]["first_hit"]
        assert c["n_traj"] == 64 and fh[37] == want and np.all(np.delete(fh, 37) == 1)
        pos = np.array([q[0] for q in c["ref"]["pos"]], dtype=np.float64)
        cheb = np.max(np.abs(c["obs"][None, :, :] - pos[:, None, :]), axis=2)
        near = (cheb < 1.0).sum(axis=1)                                                             # points in a box that covers the 27 cells
        assert near[37] == 151 and np.all(np.delete(near, 37) == 0)
        assert np.array_equal(c["obs"][-1], c["obs"][2:][np.argmin(np.abs(c["ref"]["margins"][37][0][0][2:]))])     # the decisive point comes last
