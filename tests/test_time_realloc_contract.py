"""CPU contract of the time re-allocation tests: the inputs of tests/test_gpu_time_realloc.py are what they were designed to be, and the
1e-12 relative tolerance used there on the device is a sound one for them.

The reference (tests/time_realloc_reference.py) restates the rule of include/uavqp.h in np.longdouble.  The device evaluates the same
float64 polynomials in another order (Horner, fused multiply-add): 1e-12 relative is the project's figure for that situation
(uavqp_eval_batch_device against numpy, tests/test_gpu_parity.py).  Here the kernel's float64 order, restated in numpy, must stay below
1e-13 of the reference on every designed input -- a factor 10 to spare; measured: 1.9e-16 .. 3.7e-16."""
import numpy as np
import pytest

import time_realloc_reference as R

GPU_TOL = 1e-12


def _class_counts(case):
    ref = case["ref"]
    by_speed = np.asarray(ref["rho_v"] >= ref["rho_a"])
    capped = np.asarray(ref["factor"] == R.LD(R.MAX_STRETCH))
    in_band = np.asarray((ref["rho"] > 1.001) & ~ref["stretched"])          # a dead band of 1.001 would stretch these
    return dict(n=case["n_traj"], stretched=int(ref["stretched"].sum()), by_speed=int((ref["stretched"] & by_speed).sum()),
                by_acc=int((ref["stretched"] & ~by_speed).sum()), capped=int(capped.sum()), in_band=int(in_band.sum()))


# name -> trajectories, stretched, of those decided by the speed / by the acceleration / cut off at max_stretch, left alone inside (1.001, 1.01]
DESIGNED = {
    "sweep17": dict(n=48, stretched=17, by_speed=9, by_acc=8, capped=0, in_band=15),
    "sample_axis": dict(n=48, stretched=18, by_speed=9, by_acc=9, capped=0, in_band=15),
    "ragged_mix": dict(n=80, stretched=30, by_speed=15, by_acc=15, capped=10, in_band=25),
}


@pytest.mark.parametrize("r", [3, 4])
def test_designed_inputs_are_what_they_were_designed_to_be(r):
    cases = R.designed_cases(r)
    assert set(cases) == set(DESIGNED)
    assert cases["sweep17"]["uniform"] == 17 and cases["sample_axis"]["uniform"] == 9 and cases["ragged_mix"]["uniform"] == 0
    assert set(cases["ragged_mix"]["M"]) == set(R.M_POOL)
    assert set(s["M"] for s in cases["ragged_mix"]["specs"] if s["cls"] not in ("plain", "band")) == set(R.M_POOL)
    seen_seg17, seen_site = set(), set()
    for name, case in cases.items():
        assert _class_counts(case) == DESIGNED[name], name
        ref, specs, so = case["ref"], case["specs"], case["seg_offsets64"]
        seg, smp, share = R.peak_sites(case)
        for b, s in enumerate(specs):
            planted = s["cls"] not in ("plain", "band")
            assert bool(ref["stretched"][b]) == planted, (name, b)
            # exactly one segment of duration 1.0 at least: the applied factor can be read back
            assert np.any(case["times"][so[b]:so[b + 1]] == 1.0)
            if s["cls"] == "plain":
                assert ref["rho"][b] < 0.9
                continue
            if planted:
                # the peak sits in the designed segment, at the designed sample, on the designed axis (> 95 % of the squared peak)
                want_smp = {"first": 0, "last": R.SAMPLES}.get(s["pos"], s["pos"])
                assert (seg[b], smp[b]) == (s["seg"], want_smp) and share[b][s["axis"]] > 0.95, (name, b, s, seg[b], smp[b], share[b])
                assert bool(ref["rho_v"][b] >= ref["rho_a"][b]) == (s["cls"] in ("v", "vcap")), (name, b)
                assert bool(ref["factor"][b] == R.MAX_STRETCH) == (s["cls"] in ("vcap", "acap")), (name, b)
                # unchanged neighbours on both sides inside the same wave of 8 trajectories
                assert 0 < b % 8 < 7 and not ref["stretched"][b - 1] and not ref["stretched"][b + 1]
                if name == "sweep17":
                    seen_seg17.add(s["seg"])
                if name == "sample_axis":
                    seen_site.add((s["cls"], s["pos"], s["axis"]))
    assert seen_seg17 == set(range(17))
    assert seen_site == {(c, p, a) for c in ("v", "a") for p in ("first", 11, "last") for a in range(3)}


def test_big_ragged_batch_shape_and_mix():
    case = R.big_ragged_case()
    n = case["n_traj"]
    assert n == 65536 + 11 and n % 8 != 0 and n > 256 * 32 * 8           # past one grid of an MI355X (256 CUs x 32 blocks x 8 trajectories)
    assert set(case["M"]) == {1, 2, 3} and case["r"] == 3 and case["uniform"] == 0
    assert _class_counts(case) == dict(n=65547, stretched=32569, by_speed=6649, by_acc=25920, capped=18193, in_band=0)
    # the trajectories of the grid-stride round (the last 11) hold both verdicts
    assert 0 < int(case["ref"]["stretched"][65536:].sum()) < 11


def _all_cases():
    for r in (3, 4):
        for name, case in R.designed_cases(r).items():
            yield f"r{r}-{name}", case
    yield "big", R.big_ragged_case()


def test_no_trajectory_sits_on_the_dead_band():
    """Within 1e-9 relative of the dead band the verdict could depend on rounding: none of the inputs has such a trajectory (none is
    excluded from any comparison).  The default band, and the 1.2 / 1.0 bands of the settings test."""
    for tag, case in _all_cases():
        rho = case["ref"]["rho"]
        assert np.all(np.isfinite(rho)), tag
        for band in (R.DEAD_BAND, 1.2, 1.0):
            assert float(np.min(np.abs(rho / R.LD(band) - 1))) > 1e-9, (tag, band)


def test_float64_kernel_order_agrees_with_the_longdouble_reference_ten_times_below_the_gpu_tolerance():
    worst = 0.0
    for tag, case in _all_cases():
        ref = case["ref"]
        T_k, ch_k = R.kernel_arithmetic(case["r"], case["n_traj"], case["uniform"], case["seg_offsets"], case["times"], case["coeff"])
        err = float(np.max(np.abs(T_k - ref["T_new"]) / ref["T_new"]))
        print(f"{tag}: float64 kernel order against longdouble reference {err:.3e}")
        worst = max(worst, err)
        assert np.array_equal(ch_k, ref["changed"]), tag
        assert np.array_equal(T_k[~ref["stretched"][np.repeat(np.arange(case["n_traj"]), case["M"])]],
                              case["times"][~ref["stretched"][np.repeat(np.arange(case["n_traj"]), case["M"])]]), tag
    assert worst < GPU_TOL / 10


def test_reference_handles_layouts_settings_and_non_finite_input():
    """The reference itself: uniform and CSR layouts give the same numbers; dead band = overshoot = 1 makes the factor rho; any
    non-finite coefficient or duration leaves its trajectory, and only that one, unchanged."""
    case = R.designed_cases(3)["sweep17"]
    n, T, c = case["n_traj"], case["times"], case["coeff"]
    uni = case["ref"]
    csr = R.reference(3, n, 0, case["seg_offsets"], T, c)
    assert np.array_equal(uni["T_new"], csr["T_new"]) and np.array_equal(uni["changed"], csr["changed"])
    one = R.reference(3, n, 17, None, T, c, dead_band=1.0, overshoot=1.0, max_stretch=100.0)
    assert np.array_equal(one["factor"], np.where(uni["rho"] > 1, uni["rho"], 1))
    for bad in (np.nan, np.inf, -np.inf):
        c2 = c.copy()
        b = 3                                               # a stretched trajectory; poison one coefficient of its 12th segment, z axis
        c2[3 * 6 * 17 * b + (2 * 17 + 11) * 6 + 2] = bad
        out = R.reference(3, n, 17, None, T, c2)
        assert uni["changed"][b] == 17 and out["changed"][b] == 0
        keep = np.arange(n) != b
        assert np.array_equal(out["changed"][keep], uni["changed"][keep])
        assert np.array_equal(out["T_new"][17 * b:17 * b + 17], T[17 * b:17 * b + 17].astype(R.LD))
