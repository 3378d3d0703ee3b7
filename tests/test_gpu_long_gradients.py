"""-m gpu: everything that differentiates the equality solve -- uavqp_solve_backward_device, autograd.solve_batch,
uavqp_cost_time_gradient_device, uavqp_time_optimize_device -- from 25 to 96 segments, where the planners that feed the descent
optimisers work and where test_gpu_solve_backward.py / test_gpu_time_opt.py (24 segments at the most) do not reach.

What can be wrong there and pass those: the error of the backward kernel's sequential block-Thomas sweep over up to 95 interior knots;
the indexing of its HBM workspace ws[wave][segment][field][lane] (per-wave stride max_segments * F * 64, records past 32, M below
max_segments in a ragged batch, re-use round after round); the knot derivatives read from coefficients that another forward kernel
wrote (one-lane generic above 48 segments, another host path above 63); and the same for the closed-form time gradient and the
duration optimiser built on it.

Inputs and references: long_gradient_cases.py; test_long_gradient_inputs.py shows on the CPU that the references meet, with room, every
bound asked of the device here.  Tolerances, unchanged from the short tests: grad_waypoints / grad_bc 1e-9 of max|grad| of that array
per trajectory against kkt_adjoint, on every element; grad_times within 10 x the Richardson estimate (h against h / 2, itself below
1e-5) of central differences of the binary128 minimiser on the sampled durations, and -- for the kernel alone -- of kkt_adjoint's value
on every duration, so that one wrong interior segment cannot slip between four samples.

Figures: docs/measurement_log.md, "Gradients on long trajectories" (every test prints its worst case with -s)."""
import math

import numpy as np
import pytest

import uav_motion_planning_amd as U

import long_gradient_cases as G
from test_gpu_solve_backward import Dev, to_np

pytestmark = pytest.mark.gpu
TOL = 1e-9
NAN = float("nan")


def _dev_of(ctx, case, uniform=None, max_segments=None):
    d = Dev(ctx, case["r"], case["so"], case["wp"], case["T"], case["bc"], case["uniform"] if uniform is None else uniform)
    if max_segments is not None:
        d.mmax = max_segments
    return d


def _up(d, a):
    return d.torch.from_numpy(np.ascontiguousarray(a)).to(d.dev)


def _same_bytes(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def check_gradients(oracle, case, out, label, every_duration):
    """The three outputs of one backward call against the references of the case; prints one line per trajectory, then asserts.
    Returns the worst (waypoints, bc, times on the samples / Richardson, times everywhere / Richardson)."""
    refs = G.references(oracle, case)
    g_t, g_w, g_b = out
    assert all(np.all(np.isfinite(x)) for x in out), f"{label}: an output element was left unwritten or is not finite"
    bad, worst = [], np.zeros(4)
    for b in range(case["n"]):
        s0, s1 = int(case["so"][b]), int(case["so"][b + 1])
        rT, rW, rB = refs[b]["kkt"]
        idx, phi, rich = refs[b]["idx"], refs[b]["phi"], refs[b]["rich"]
        dT, dW, dB = g_t[s0:s1], g_w[s0 + b:s1 + b + 1], g_b[b]
        ew = np.max(np.abs(dW - rW)) / np.max(np.abs(rW))
        eb = np.max(np.abs(dB - rB)) / np.max(np.abs(rB))
        scale = np.max(np.abs(rT))
        es = np.max(np.abs(dT[idx] - phi[:, 1])) / scale
        ea = np.max(np.abs(dT - rT)) / scale
        print(f"  {label} {case['name']} trajectory {b} (r={case['r']}, M={s1 - s0}): waypoints {ew:.3e}, bc {eb:.3e}; times |device - fd| {es:.3e} "
              f"on {idx.size} samples, |device - kkt_adjoint| {ea:.3e} on all, Richardson estimate {rich:.3e}")
        worst = np.maximum(worst, [ew, eb, es / rich, ea / rich])
        if ew > TOL:
            bad.append(f"trajectory {b} (M={s1 - s0}): grad_waypoints {ew:.3e}, first at knot {int(np.argmax(np.abs(dW - rW).max(axis=1) > TOL * np.max(np.abs(rW))))}")
        if eb > TOL:
            bad.append(f"trajectory {b} (M={s1 - s0}): grad_bc {eb:.3e}")
        if not rich < 1e-5:
            bad.append(f"trajectory {b}: the finite-difference step is badly chosen ({rich:.3e})")
        if es > 10.0 * rich:
            bad.append(f"trajectory {b} (M={s1 - s0}): grad_times on the samples {es:.3e} vs Richardson {rich:.3e}")
        if every_duration and ea > 10.0 * rich:
            bad.append(f"trajectory {b} (M={s1 - s0}): grad_times {ea:.3e} vs Richardson {rich:.3e}, worst at segment {int(np.argmax(np.abs(dT - rT)))}")
    assert not bad, f"{label} {case['name']}: " + "; ".join(bad)
    return worst


# ---- (a) the backward kernel alone: the oracle's coefficients in, no status ------------------------------------------------------------
@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_backward_kernel_alone_on_the_oracle_coefficients(gpu_ctx, oracle, name):
    case = G.case_by_name(name)
    outs = {}
    for uniform in ((True, False) if case["uniform"] else (False,)):
        d = _dev_of(gpu_ctx, case, uniform)
        coeff = _up(d, G.oracle_coefficients(oracle, case))
        outs[uniform] = [to_np(x) for x in d.backward(coeff, case["g"], status=None, fill=NAN)]
        worst = check_gradients(oracle, case, outs[uniform], "(a) " + ("uniform dispatch" if uniform else "CSR offsets"), every_duration=True)
    print(f"(a) {name}: worst waypoints {worst[0]:.3e}, bc {worst[1]:.3e}, times {worst[2]:.2f} x Richardson on the samples, {worst[3]:.2f} x on all")
    if case["uniform"]:
        assert _same_bytes(outs[True], outs[False]), "uniform dispatch and CSR offsets give different bytes"


# ---- (b) the backward on the device's own coefficients ---------------------------------------------------------------------------------
def _solve_and_backward(ctx, oracle, case, label):
    d = _dev_of(ctx, case)
    coeff, st = d.solve()
    assert np.all(to_np(st) == U.UAVQP_SOLVED), to_np(st)
    ref = G.oracle_coefficients(oracle, case)
    cerr = np.max(np.abs(to_np(coeff) - ref)) / np.max(np.abs(ref))
    out = [to_np(x) for x in d.backward(coeff, case["g"], status=st, fill=NAN)]
    worst = check_gradients(oracle, case, out, label, every_duration=False)
    print(f"{label} {case['name']}: forward coefficients {cerr:.3e} from the oracle; worst waypoints {worst[0]:.3e}, bc {worst[1]:.3e}, "
          f"times {worst[2]:.2f} x Richardson on the samples ({worst[3]:.2f} x on all, not asserted)")
    return out


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_backward_on_the_device_coefficients(gpu_ctx, oracle, name):
    _solve_and_backward(gpu_ctx, oracle, G.case_by_name(name), "(b)")


@pytest.mark.parametrize("name", G.LANE_NAMES)
def test_backward_behind_every_lane_layout_of_the_forward(gpu_ctx, oracle, name):
    """uavqp_settings.generic_lanes_per_traj 1 / 2 / 3 at lengths the pair kernel does not take (as
    test_gpu_long_trajectories.py::test_equality_solve_lane_layouts_beyond_the_pair_kernel): the same bounds behind each."""
    case = G.case_by_name(name)
    try:
        for lanes in (1, 2, 3):
            gpu_ctx.set_settings(generic_lanes_per_traj=lanes)
            _solve_and_backward(gpu_ctx, oracle, case, f"(b) lanes {lanes}")
    finally:
        gpu_ctx.set_settings(generic_lanes_per_traj=0)


# ---- (c) layout properties of the ragged batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,M", [(3, 33), (3, 64)])
def test_uniform_batch_as_csr_gives_the_same_bytes(gpu_ctx, r, M):
    case = G.uniform_case(r, M)
    du, dc = _dev_of(gpu_ctx, case, True), _dev_of(gpu_ctx, case, False)
    coeff, st = du.solve()
    assert np.all(to_np(st) == U.UAVQP_SOLVED)
    a = [to_np(x) for x in du.backward(coeff, case["g"], status=st, fill=NAN)]
    b = [to_np(x) for x in dc.backward(coeff, case["g"], status=st, fill=NAN)]
    assert all(np.all(np.isfinite(x)) for x in a + b)
    assert _same_bytes(a, b)


def _slices(case, b):
    s0, s1 = int(case["so"][b]), int(case["so"][b + 1])
    return slice(s0, s1), slice(s0 + b, s1 + b + 1), b


@pytest.mark.parametrize("r", [3, 4])
def test_ragged_batch_each_trajectory_alone_and_under_a_smaller_max_segments(gpu_ctx, oracle, r):
    case = G.ragged_case(r)
    nc = 2 * r
    ref_c = G.oracle_coefficients(oracle, case)
    d = _dev_of(gpu_ctx, case)
    assert d.mmax == G.RAGGED_MAX
    coeff = _up(d, ref_c)
    whole = [to_np(x) for x in d.backward(coeff, case["g"], status=None, fill=NAN)]
    assert all(np.all(np.isfinite(x)) for x in whole), "an output element was left unwritten"
    # each trajectory alone, its own max_segments: a record stride that depends on max_segments the wrong way shows here
    for b in range(case["n"]):
        M, wp, bc, T, g = G.traj(case, b)
        st_, sw_, _ = _slices(case, b)
        solo = Dev(gpu_ctx, r, np.array([0, M], dtype=np.int32), wp, T, bc[None], False)
        assert solo.mmax == M and solo.n == 1
        c_b = _up(solo, ref_c[3 * nc * st_.start:3 * nc * st_.stop])
        alone = [to_np(x) for x in solo.backward(c_b, g.ravel(), status=None, fill=NAN)]
        assert _same_bytes(alone, (whole[0][st_], whole[1][sw_], whole[2][b:b + 1])), f"trajectory {b} (M={M}) alone differs from the batch"
    # max_segments = 64: the 96-segment trajectory gets exactly zero (include/uavqp.h: "M > max_segments: zeros"), the others do not change
    small = [to_np(x) for x in _dev_of(gpu_ctx, case, max_segments=64).backward(coeff, case["g"], status=None, fill=NAN)]
    for b in range(case["n"]):
        st_, sw_, _ = _slices(case, b)
        mine, theirs = (small[0][st_], small[1][sw_], small[2][b]), (whole[0][st_], whole[1][sw_], whole[2][b])
        if case["lengths"][b] > 64:
            assert all(np.all(x == 0.0) for x in mine), f"trajectory {b} is longer than max_segments: zeros"
        else:
            assert _same_bytes(mine, theirs), f"trajectory {b} (M={case['lengths'][b]}) changes with max_segments"
    assert np.any(whole[0][_slices(case, 6)[0]] != 0.0)
    # the batch nine times over: 72 trajectories, the last eight in a second wave, whose workspace starts max_segments records behind
    # the first one's; every copy gives the bytes of the original
    reps, lens = 9, case["lengths"]
    so9 = np.concatenate([[0], np.cumsum(np.tile(lens, reps))]).astype(np.int32)
    d9 = Dev(gpu_ctx, r, so9, np.tile(case["wp"], (reps, 1)), np.tile(case["T"], reps), np.tile(case["bc"], (reps, 1, 1, 1)), False)
    tiled = [to_np(x) for x in d9.backward(_up(d9, np.tile(ref_c, reps)), np.tile(case["g"], reps), status=None, fill=NAN)]
    for k in range(reps):
        assert _same_bytes([x.reshape((reps, -1) + x.shape[1:])[k] for x in tiled], whole), f"copy {k} of the batch differs from the batch alone"


def test_ragged_batch_between_guard_bands(gpu_ctx, oracle):
    from test_gpu_guard_bands import Arena, _both_fills
    r = 4
    case = G.ragged_case(r)
    n, total = case["n"], int(case["so"][-1])
    ref_c = G.oracle_coefficients(oracle, case)

    def run_long_backward(ar):
        d_so, d_wp, d_T, d_bc = ar.put(case["so"]), ar.put(case["wp"]), ar.put(case["T"]), ar.put(case["bc"])
        coeff, g = ar.put(ref_c), ar.put(case["g"])
        out = {}
        for mx in (G.RAGGED_MAX, 64):
            g_t, g_w, g_b = ar.out(total, misalign=8), ar.out((total + n, 3)), ar.out((n, 2, r - 1, 3), misalign=8)
            gpu_ctx.solve_backward_device(r, n, 0, mx, total, d_so, d_wp, d_T, d_bc, coeff, g, grad_times=g_t, grad_waypoints=g_w, grad_bc=g_b)
            out.update({f"g_t{mx}": g_t, f"g_w{mx}": g_w, f"g_b{mx}": g_b})
        # and behind the forward, which writes the coefficients and the status inside the arena
        c2, st = ar.out(3 * 2 * r * total), ar.out(n, np.int32)
        gpu_ctx.solve_batch_device(r, n, 0, G.RAGGED_MAX, d_so, d_wp, d_T, d_bc, c2, st)
        g_t, g_w, g_b = ar.out(total), ar.out((total + n, 3), misalign=8), ar.out((n, 2, r - 1, 3))
        gpu_ctx.solve_backward_device(r, n, 0, G.RAGGED_MAX, total, d_so, d_wp, d_T, d_bc, c2, g, grad_times=g_t, grad_waypoints=g_w, grad_bc=g_b, status=st)
        gpu_ctx.synchronize()
        out.update(g_t=g_t, g_w=g_w, g_b=g_b, st=st)
        return out
    res = _both_fills(run_long_backward)
    assert np.all(res["st"] == U.UAVQP_SOLVED)
    assert np.all(res["g_t96"] != 0.0) and np.all(res["g_t"] != 0.0)


# ---- (d) grid-stride rounds with interior knots ----------------------------------------------------------------------------------------
def test_grid_stride_rounds_with_interior_knots(gpu_ctx):
    """test_gpu_solve_backward.py::test_grid_stride_rounds_equal_separate_launches with M cycling 1, 2, 3, 4: with one segment the kernel
    never touches a workspace record of an interior knot, so that test does not see a record re-used round after round.  40000
    trajectories in one launch (more than 64 x 2 x the number of CUs) give the bytes of two launches of 20000 (a single round each)."""
    r, n = 3, 40000
    nc = 2 * r
    rng = np.random.default_rng(23)
    lens = np.tile(np.array([1, 2, 3, 4]), n // 4)
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    total = int(so[-1])
    wp = np.cumsum(rng.normal(size=(total + n, 3)), axis=0)
    T = rng.uniform(0.7, 2.0, size=total)
    bc = rng.normal(size=(n, 2, r - 1, 3))
    g = rng.normal(size=3 * nc * total)
    whole = Dev(gpu_ctx, r, so, wp, T, bc, False)
    coeff, st = whole.solve()
    assert np.all(to_np(st) == U.UAVQP_SOLVED)
    got = [to_np(x) for x in whole.backward(coeff, g, status=st, fill=NAN)]
    assert all(np.all(np.isfinite(x)) for x in got) and np.all(got[0] != 0.0)
    h = n // 2
    for lo in (0, h):
        s0, s1 = int(so[lo]), int(so[lo + h])
        part = Dev(gpu_ctx, r, so[lo:lo + h + 1] - so[lo], wp[s0 + lo:s1 + lo + h], T[s0:s1], bc[lo:lo + h], False)
        assert part.total == s1 - s0 and part.mmax == 4
        ref = [to_np(x) for x in part.backward(coeff[3 * nc * s0:3 * nc * s1].clone(), g[3 * nc * s0:3 * nc * s1], status=st[lo:lo + h].clone(), fill=NAN)]
        assert _same_bytes(ref, (got[0][s0:s1], got[1][s0 + lo:s1 + lo + h], got[2][lo:lo + h])), f"launch of trajectories {lo} .. {lo + h} differs"


# ---- (e) cost and closed-form time gradient ---------------------------------------------------------------------------------------------
def _cost_grad(ctx, d, coeff, d_T=None):
    t = d.torch
    cost = t.full((d.n,), NAN, dtype=t.float64, device=d.dev)
    grad = t.full((d.total,), NAN, dtype=t.float64, device=d.dev)
    ctx.cost_time_gradient_device(d.r, d.n, d.uni, d.d_so, d.d_T if d_T is None else d_T, coeff, cost, grad)
    ctx.synchronize()
    return to_np(cost), to_np(grad)


@pytest.mark.parametrize("name", ["uniform_r3_M49", "uniform_r4_M63", "uniform_r4_M96", "ragged_r3", "ragged_r4"])
def test_cost_and_time_gradient_on_long_trajectories(gpu_ctx, oracle, name):
    case = G.case_by_name(name)
    r, nc = case["r"], 2 * case["r"]
    d = _dev_of(gpu_ctx, case)
    coeff, st = d.solve()
    assert np.all(to_np(st) == U.UAVQP_SOLVED)
    cost, grad = _cost_grad(gpu_ctx, d, coeff)
    c_np = to_np(coeff)
    refs = G.references(oracle, case)
    worst_c = worst_g = worst_rich = 0.0
    for b in range(case["n"]):
        sl, _, _ = _slices(case, b)
        # the cost of the SAME coefficients in extended precision (test_gpu_time_opt.py::test_cost_vs_oracle's 1e-9)
        P, _ = oracle.assemble(r, case["T"][sl])
        c = c_np[3 * nc * sl.start:3 * nc * sl.stop].reshape(3, -1).astype(np.longdouble)
        want = float(np.sum((c @ P.astype(np.longdouble)) * c))
        worst_c = max(worst_c, abs(cost[b] - want) / want)
        # the gradient on the sampled durations: central differences of the oracle's optimal cost, Richardson rule
        idx, J = refs[b]["idx"], refs[b]["J"]
        scale = np.max(np.abs(J[:, 1]))
        rich = np.max(np.abs(J[:, 0] - J[:, 1])) / scale
        err = np.max(np.abs(grad[sl][idx] - J[:, 1])) / scale
        print(f"  (e) {name} trajectory {b} (M={sl.stop - sl.start}): cost {abs(cost[b] - want) / want:.3e}; gradient |device - fd| {err:.3e}, Richardson {rich:.3e}")
        worst_g, worst_rich = max(worst_g, err / rich), max(worst_rich, rich)
        assert rich < 1e-5, f"trajectory {b}: the finite-difference step is badly chosen ({rich:.3e})"
        assert err <= 10.0 * rich, f"trajectory {b}: dJ/dT {err:.3e} vs Richardson {rich:.3e}"
    assert worst_c <= 1e-9, worst_c
    # homogeneity (test_gpu_time_opt.py::test_homogeneity_identity): zero boundary derivatives, sum_i T_i dJ/dT_i = -(2r - 1) J
    d0 = Dev(gpu_ctx, r, case["so"], case["wp"], case["T"], np.zeros_like(case["bc"]), case["uniform"])
    c0, st0 = d0.solve()
    assert np.all(to_np(st0) == U.UAVQP_SOLVED)
    cost0, grad0 = _cost_grad(gpu_ctx, d0, c0)
    lhs = np.add.reduceat(case["T"] * grad0, case["so"][:-1])
    hom = np.max(np.abs(lhs + (2 * r - 1) * cost0) / ((2 * r - 1) * cost0))
    print(f"(e) {name}: cost max rel err {worst_c:.3e}, gradient {worst_g:.2f} x Richardson (largest estimate {worst_rich:.3e}), homogeneity {hom:.3e}")
    assert hom <= 1e-9, hom


@pytest.mark.parametrize("r,M", [(3, 49), (3, 64)])
def test_tie_to_the_closed_form_time_gradient_on_long_trajectories(gpu_ctx, oracle, r, M):
    """test_gpu_solve_backward.py::test_tie_to_the_closed_form_time_gradient: g = 2 P c*, through part (the backward) + explicit part
    sum over axes (p^(r)(T_i))^2 = the closed form of uavqp_cost_time_gradient_device, at 1e-9 of the largest term per trajectory."""
    case = G.uniform_case(r, M)
    nc = 2 * r
    d = _dev_of(gpu_ctx, case)
    coeff, st = d.solve()
    assert np.all(to_np(st) == U.UAVQP_SOLVED)
    c_np = to_np(coeff)
    g, explicit = np.zeros_like(c_np), np.zeros(d.total)
    k = np.arange(r, nc)
    fall = np.array([math.factorial(int(j)) / math.factorial(int(j) - r) for j in k])
    for b in range(d.n):
        sl, _, _ = _slices(case, b)
        T_b = case["T"][sl]
        P, _ = oracle.assemble(r, T_b)
        c = c_np[3 * nc * sl.start:3 * nc * sl.stop].reshape(3, -1)
        g[3 * nc * sl.start:3 * nc * sl.stop] = (2.0 * c @ P).ravel()
        pr = np.einsum("aik,ik->ai", c.reshape(3, M, nc)[:, :, r:] * fall, T_b[:, None] ** (k - r)[None, :])
        explicit[sl] = np.sum(pr ** 2, axis=0)
    through = to_np(d.backward(coeff, g, status=st, want=(True, False, False), fill=NAN)[0])
    _, closed = _cost_grad(gpu_ctx, d, coeff)
    worst = 0.0
    for b in range(d.n):
        sl, _, _ = _slices(case, b)
        scale = max(np.max(np.abs(closed[sl])), np.max(explicit[sl]), np.max(np.abs(through[sl])))
        worst = max(worst, np.max(np.abs(through[sl] + explicit[sl] - closed[sl])) / scale)
    print(f"(e) r={r} M={M}: max |through + explicit - closed form| / max term = {worst:.3e}")
    assert worst <= 1e-9


# ---- (f) autograd and the duration optimiser --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform_r4_M63", "ragged_r3", "ragged_r4"])
def test_autograd_reproduces_the_c_abi_bitwise_on_long_trajectories(gpu_ctx, name):
    import torch
    from uav_motion_planning_amd.autograd import solve_batch
    case = G.case_by_name(name)
    r = case["r"]
    d = _dev_of(gpu_ctx, case)
    coeff_ref, st = d.solve()
    assert np.all(to_np(st) == U.UAVQP_SOLVED)
    g = _up(d, case["g"])
    ref = d.backward(coeff_ref, g, status=st, fill=NAN)
    wp, T, bc = (x.clone().requires_grad_(True) for x in (d.d_wp, d.d_T, d.d_bc))
    try:
        coeff = solve_batch(gpu_ctx, r, wp, T, bc, seg_offsets=None if case["uniform"] else d.d_so, uniform_segments=d.uni, check_status=True)
        assert torch.equal(coeff.detach(), coeff_ref)
        (coeff * g).sum().backward()
        torch.cuda.synchronize()
    finally:
        gpu_ctx.set_stream(None)
    assert torch.equal(T.grad, ref[0]) and torch.equal(wp.grad, ref[1]) and torch.equal(bc.grad, ref[2])
    assert bool(torch.isfinite(T.grad).all()) and bool((T.grad != 0.0).all())


def _optimiser_batches():
    out = {f"uniform_r4_M{M}": G.uniform_case(4, M, n=4) for M in (48, 49, 64)}
    out.update(ragged_r3=G.ragged_case(3), ragged_r4=G.ragged_case(4))
    return out


@pytest.mark.parametrize("name", ["uniform_r4_M48", "uniform_r4_M49", "uniform_r4_M64", "ragged_r3", "ragged_r4"])
def test_duration_optimiser_contract_on_long_trajectories(gpu_ctx, name):
    """The contract of test_gpu_time_opt.py::test_optimiser_contract, default parameters."""
    from test_gpu_time_opt import Dev as TimeDev, defaults
    case = _optimiser_batches()[name]
    d = TimeDev(gpu_ctx, dict(r=case["r"], seg_offsets=case["so"], waypoints=case["wp"], times=case["T"], bc=case["bc"]), case["uniform"])
    P = defaults()
    d_T, coeff, status, obj, acc = d.optimize()
    T = d_T.cpu().numpy()
    assert np.all(status.cpu().numpy() == U.UAVQP_SOLVED), status
    print(f"(f) {name}: f_result / f_start {np.array2string(obj[:, 1] / obj[:, 0], precision=3)}, accepted trials {acc}")
    assert np.all(np.isfinite(obj)) and np.all(obj[:, 1] <= obj[:, 0])
    assert np.all(T >= P.t_min) and np.all(T <= P.t_max)
    assert np.all(acc >= 0) and np.all(acc <= P.max_iters)
    assert np.all(acc >= 1), "a trajectory never accepted a trial"
    cost, _ = d.cost_grad(d_T, coeff)
    f = cost + P.time_weight * np.add.reduceat(T, d.so[:-1])
    assert np.max(np.abs(f - obj[:, 1]) / obj[:, 1]) <= 1e-12
    fresh, st2 = d.solve(d_T)
    assert np.array_equal(fresh.cpu().numpy(), coeff.cpu().numpy()) and np.all(st2.cpu().numpy() == U.UAVQP_SOLVED)
