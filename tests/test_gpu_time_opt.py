"""-m gpu: control cost, exact time gradient and the duration optimiser (uavqp_cost_time_gradient_device, uavqp_time_optimize_*)
against the CPU oracle.

J = c' P c = sum over axes and segments of integral (p^(r))^2 -- TWICE oracle.cost, which is OSQP's objective 1/2 x' P x per axis.
Tolerances: cost and the homogeneity identity 1e-9 relative (the project's coefficient parity tolerance: the cost is stationary at the
minimiser, its error is second order in the coefficient error plus the rounding of the sum); the gradient against central differences of
the oracle's optimal cost within 10 x the scheme's own error, which the test estimates at run time (Richardson: h against h / 2); the
optimiser within 5 % of the decrease scipy's L-BFGS-B attains on the oracle's objective.

Measured on MI355X (docs/measurement_log.md, "Time optimisation"): see there."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

import uav_motion_planning_amd as U
from uav_motion_planning_amd import _lib
from uav_motion_planning_amd import workloads as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "kkt_exact.json")))["cases"]
C_R = {3: 720.0, 4: 100800.0}   # single rest-to-rest segment: J = C_r |D|^2 / T^(2r-1)


def defaults():
    p = _lib.TimeOptParams()
    _lib.lib().uavqp_default_time_opt_params(ctypes.byref(p))
    return p


def flat_batch(b, uniform):
    """-> (r, n_traj, uniform_segments, max_segments, so [n+1] int32, waypoints, times, bc) as flat float64 arrays"""
    so = np.ascontiguousarray(b["seg_offsets"], dtype=np.int32)
    n = so.size - 1
    mmax = int(np.max(np.diff(so)))
    return (b["r"], n, (mmax if uniform else 0), mmax, so, np.ascontiguousarray(b["waypoints"], dtype=np.float64).reshape(-1, 3),
            np.ascontiguousarray(b["times"], dtype=np.float64).ravel(), np.ascontiguousarray(b["bc"], dtype=np.float64))


class Dev:
    """One batch on the device: solve, cost + gradient, optimise (all through the device-pointer entries)."""

    def __init__(self, ctx, b, uniform):
        import torch
        self.torch, self.ctx = torch, ctx
        self.r, self.n, self.uni, self.mmax, self.so, wp, T, bc = flat_batch(b, uniform)
        dev = torch.device("cuda", 0)
        self.total = int(self.so[-1])
        self.d_so = torch.from_numpy(self.so).to(dev)
        self.d_wp = torch.from_numpy(wp).to(dev)
        self.d_bc = torch.from_numpy(bc).to(dev)
        self.T0 = T
        self.dev = dev

    def times(self, T=None):
        return self.torch.from_numpy(np.ascontiguousarray(self.T0 if T is None else T)).to(self.dev)

    def solve(self, d_T):
        t = self.torch
        coeff = t.zeros(3 * 2 * self.r * self.total, dtype=t.float64, device=self.dev)
        status = t.zeros(self.n, dtype=t.int32, device=self.dev)
        t.cuda.synchronize()
        self.ctx.solve_batch_device(self.r, self.n, self.uni, self.mmax, self.d_so, self.d_wp, d_T, self.d_bc, coeff, status)
        self.ctx.synchronize()
        return coeff, status

    def cost_grad(self, d_T, coeff):
        t = self.torch
        cost = t.zeros(self.n, dtype=t.float64, device=self.dev)
        grad = t.zeros(self.total, dtype=t.float64, device=self.dev)
        t.cuda.synchronize()
        self.ctx.cost_time_gradient_device(self.r, self.n, self.uni, self.d_so, d_T, coeff, cost, grad)
        self.ctx.synchronize()
        return cost.cpu().numpy(), grad.cpu().numpy()

    def optimize(self, T=None, **params):
        t = self.torch
        d_T = self.times(T)
        coeff = t.zeros(3 * 2 * self.r * self.total, dtype=t.float64, device=self.dev)
        status = t.zeros(self.n, dtype=t.int32, device=self.dev)
        obj = t.zeros((self.n, 2), dtype=t.float64, device=self.dev)
        acc = t.zeros(self.n, dtype=t.int32, device=self.dev)
        t.cuda.synchronize()
        self.ctx.time_optimize_device(self.r, self.n, self.uni, self.mmax, self.total, self.d_so, self.d_wp, d_T, self.d_bc, coeff, status,
                                      obj, acc, **params)
        self.ctx.synchronize()
        return d_T, coeff, status, obj.cpu().numpy(), acc.cpu().numpy()


def oracle_costs(oracle, r, so, T, coef_ref):
    """[n] c' P c of the oracle's minimiser (2 x oracle.cost per axis)"""
    nc = 2 * r
    out = np.zeros(so.size - 1)
    for b in range(so.size - 1):
        s0, s1 = int(so[b]), int(so[b + 1])
        c = coef_ref[3 * nc * s0:3 * nc * s1].reshape(3, -1)
        out[b] = sum(2.0 * oracle.cost(r, T[s0:s1], c[ax]) for ax in range(3))
    return out


def batches():
    return {
        "config2_4096x8_r4": (W.uniform_batch(2, 4096, 8, 4, time_mode="distance"), True),
        "ragged_r3_M1to24": (W.ragged_batch(4, 512, 3, m_lo=1, m_hi=24), False),
    }


@pytest.mark.parametrize("name", ["config2_4096x8_r4", "ragged_r3_M1to24"])
def test_cost_vs_oracle(gpu_ctx, oracle, name):
    b, uniform = batches()[name]
    d = Dev(gpu_ctx, b, uniform)
    d_T = d.times()
    coeff, st = d.solve(d_T)
    assert np.all(st.cpu().numpy() == U.UAVQP_SOLVED)
    cost, _ = d.cost_grad(d_T, coeff)
    ref, st_ref = oracle.solve_exact_batch(d.r, d.so, b["waypoints"], b["times"], b["bc"])
    assert np.all(st_ref == 0)
    want = oracle_costs(oracle, d.r, d.so, d.T0, ref)
    err = np.abs(cost - want) / want
    print(f"{name}: cost max rel err vs oracle {err.max():.3e}")
    assert err.max() <= 1e-9


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cost_on_the_golden_shapes(gpu_ctx, oracle, case):
    r, M, n = case["r"], case["M"], 5
    b = dict(r=r, seg_offsets=(np.arange(n + 1) * M).astype(np.int32), waypoints=np.tile(np.array(case["waypoints"])[None], (n, 1, 1)),
             times=np.tile(np.array(case["times"])[None], (n, 1)), bc=np.tile(np.array(case["bc"])[None], (n, 1, 1, 1)))
    d = Dev(gpu_ctx, b, True)
    d_T = d.times()
    coeff, st = d.solve(d_T)
    assert np.all(st.cpu().numpy() == U.UAVQP_SOLVED)
    cost, _ = d.cost_grad(d_T, coeff)
    ref, _ = oracle.solve_exact_batch(r, d.so, b["waypoints"], b["times"], b["bc"])
    want = oracle_costs(oracle, r, d.so, d.T0, ref)
    exact = 2.0 * sum(case["half_xPx"])      # the fixture's exact-rational 1/2 x' P x per axis
    print(f"{case['name']}: cost rel err vs oracle {np.max(np.abs(cost - want) / want):.3e}, vs the fixture {np.max(np.abs(cost - exact)) / exact:.3e}")
    assert np.max(np.abs(cost - want) / want) <= 1e-9
    assert np.max(np.abs(cost - exact)) / exact <= 1e-9


@pytest.mark.parametrize("name", ["config2_4096x8_r4", "ragged_r3_M1to24"])
def test_homogeneity_identity(gpu_ctx, name):
    """All boundary derivatives zero: J(sT) = s^-(2r-1) J(T), hence sum_i T_i dJ/dT_i = -(2r-1) J.  Device output only, full size."""
    b, uniform = batches()[name]
    b = dict(b, bc=np.zeros_like(b["bc"]))
    d = Dev(gpu_ctx, b, uniform)
    d_T = d.times()
    coeff, st = d.solve(d_T)
    assert np.all(st.cpu().numpy() == U.UAVQP_SOLVED)
    cost, grad = d.cost_grad(d_T, coeff)
    lhs = np.add.reduceat(d.T0 * grad, d.so[:-1])
    err = np.abs(lhs + (2 * d.r - 1) * cost) / ((2 * d.r - 1) * cost)
    print(f"{name}: homogeneity max rel err {err.max():.3e}")
    assert err.max() <= 1e-9


def gradient_subset():
    """64 trajectories: uniform / ragged, r = 3 / 4, M = 1 included, non-zero boundary derivatives at both ends"""
    rng = np.random.default_rng(77)
    out = []
    for b, uniform in ((W.uniform_batch(2, 16, 8, 4, time_mode="distance"), True), (W.uniform_batch(1, 16, 1, 3, time_mode="distance"), True),
                       (W.ragged_batch(4, 16, 3, m_lo=1, m_hi=6), False), (W.ragged_batch(5, 16, 4, m_lo=1, m_hi=6), False)):
        bc = np.array(b["bc"], dtype=np.float64)
        bc += rng.uniform(-1.0, 1.0, size=bc.shape)
        out.append((dict(b, bc=bc), uniform))
    return out


def test_gradient_vs_central_differences_of_the_oracle(gpu_ctx, oracle):
    H_REL = 1e-4     # step relative to T_i (the scheme's error at this step comes out ~1e-7: measured below, must stay under 1e-5)
    worst_err, worst_rich, count = 0.0, 0.0, 0
    for b, uniform in gradient_subset():
        d = Dev(gpu_ctx, b, uniform)
        d_T = d.times()
        coeff, st = d.solve(d_T)
        assert np.all(st.cpu().numpy() == U.UAVQP_SOLVED)
        _, grad = d.cost_grad(d_T, coeff)
        wp = np.asarray(b["waypoints"], dtype=np.float64).reshape(-1, 3)
        for t in range(d.n):
            s0, s1 = int(d.so[t]), int(d.so[t + 1])
            M = s1 - s0
            w_t, bc_t, T_t = wp[s0 + t:s1 + t + 1], b["bc"][t], d.T0[s0:s1]

            def J(T):
                return sum(2.0 * oracle.cost(d.r, T, oracle.solve_exact(d.r, w_t[:, ax], bc_t[0, :, ax], bc_t[1, :, ax], T)) for ax in range(3))

            def fd(h):
                g = np.zeros(M)
                for i in range(M):
                    e = np.zeros(M)
                    e[i] = h * T_t[i]
                    g[i] = (J(T_t + e) - J(T_t - e)) / (2.0 * e[i])
                return g
            g1, g2 = fd(H_REL), fd(H_REL / 2)
            scale = np.max(np.abs(g2))
            worst_rich = max(worst_rich, np.max(np.abs(g1 - g2)) / scale)
            worst_err = max(worst_err, np.max(np.abs(grad[s0:s1] - g2)) / scale)
            count += 1
    print(f"gradient: {count} trajectories, max |device - central difference| / max|grad| = {worst_err:.3e}; "
          f"the scheme's own error (h = {H_REL} T_i against h / 2) = {worst_rich:.3e}")
    assert count >= 64
    assert worst_rich < 1e-5, "the finite-difference step is badly chosen"
    assert worst_err <= 10.0 * worst_rich


@pytest.mark.parametrize("name", ["config2_4096x8_r4", "ragged_r3_M1to24"])
def test_optimiser_contract(gpu_ctx, name):
    b, uniform = batches()[name]
    d = Dev(gpu_ctx, b, uniform)
    P = defaults()
    bad = 5                                             # one invalid trajectory among valid neighbours
    T0 = d.T0.copy()
    T0[int(d.so[bad])] = -1.0
    d_T, coeff, status, obj, acc = d.optimize(T0)
    T = d_T.cpu().numpy()
    st = status.cpu().numpy()
    ok = np.ones(d.n, dtype=bool)
    ok[bad] = False
    seg_ok = np.repeat(ok, np.diff(d.so))
    assert np.all(st[ok] == U.UAVQP_SOLVED) and st[bad] == U.UAVQP_INVALID_INPUT
    assert np.array_equal(T[~seg_ok], T0[~seg_ok]), "an invalid trajectory keeps its durations"
    assert np.all(np.isnan(obj[bad])) and acc[bad] == 0
    assert np.all(obj[ok, 1] <= obj[ok, 0])
    assert np.all(T[seg_ok] >= P.t_min) and np.all(T[seg_ok] <= P.t_max)
    assert np.all(acc >= 0) and np.all(acc <= P.max_iters)
    assert np.median(obj[ok, 1] / obj[ok, 0]) < 1.0, "the optimiser did not move"
    # self-consistent: the coefficients are a plain solve at the durations handed back, the objective is recomputed from them
    fresh, st2 = d.solve(d_T)
    assert np.array_equal(fresh.cpu().numpy(), coeff.cpu().numpy()) and np.array_equal(st2.cpu().numpy(), st)
    cost, _ = d.cost_grad(d_T, coeff)
    f = cost + P.time_weight * np.add.reduceat(T, d.so[:-1])
    assert np.max(np.abs(f[ok] - obj[ok, 1]) / obj[ok, 1]) <= 1e-12
    # run to run: identical bytes
    d_T2, coeff2, status2, obj2, acc2 = d.optimize(T0)
    assert np.array_equal(d_T2.cpu().numpy(), T) and np.array_equal(coeff2.cpu().numpy(), coeff.cpu().numpy())
    assert np.array_equal(obj2[ok], obj[ok]) and np.array_equal(acc2, acc) and np.array_equal(status2.cpu().numpy(), st)
    # max_iters = 0: the plain solve
    d_T3, coeff3, status3, obj3, acc3 = d.optimize(T0, max_iters=0)
    plain, st_plain = d.solve(d.times(T0))
    assert np.array_equal(d_T3.cpu().numpy(), T0)
    assert np.array_equal(coeff3.cpu().numpy(), plain.cpu().numpy()) and np.array_equal(status3.cpu().numpy(), st_plain.cpu().numpy())
    assert np.array_equal(obj3[ok, 0], obj3[ok, 1]) and np.array_equal(obj3[ok, 0], obj[ok, 0]) and np.all(acc3 == 0)
    print(f"{name}: median f_result / f_start {np.median(obj[ok, 1] / obj[ok, 0]):.3f}, accepted trials min / median / max "
          f"{acc[ok].min()} / {int(np.median(acc[ok]))} / {acc[ok].max()}")


def test_params_are_validated(gpu_ctx):
    b, uniform = W.uniform_batch(2, 8, 4, 3, time_mode="distance"), True
    d = Dev(gpu_ctx, b, uniform)
    for bad in (dict(time_weight=0.0), dict(time_weight=-1.0), dict(t_min=0.0), dict(t_min=2.0, t_max=1.0), dict(max_iters=-1),
                dict(initial_step=0.0), dict(armijo_c=1.0), dict(shrink=1.0), dict(grow=0.5), dict(time_weight=math.inf)):
        with pytest.raises(U.UavqpError):
            d.optimize(**bad)
    with pytest.raises(ValueError):
        d.optimize(struct_size=4)


@pytest.mark.parametrize("r", [3, 4])
def test_optimiser_reaches_the_closed_form_optimum_of_one_segment(gpu_ctx, r):
    """Rest-to-rest over D in one segment: J = C_r |D|^2 / T^(2r-1), f = J + w T is minimal at T* = ((2r-1) C_r |D|^2 / w)^(1/2r).
    Same condition as against scipy below: at most 5 % of the attainable decrease left, on every trajectory that has one to speak of."""
    n = 64
    rng = np.random.default_rng(5 + r)
    dist = np.logspace(-0.5, 1.5, n)
    dirs = rng.normal(size=(n, 3))
    wp = np.zeros((n, 2, 3))
    wp[:, 1] = dirs / np.linalg.norm(dirs, axis=1)[:, None] * dist[:, None]
    b = dict(r=r, seg_offsets=np.arange(n + 1, dtype=np.int32), waypoints=wp, times=np.ones((n, 1)), bc=np.zeros((n, 2, r - 1, 3)))
    d = Dev(gpu_ctx, b, True)
    checked, worst_gap, worst_T = 0, 0.0, 0.0
    for w in (1.0, 50.0, 1000.0):
        d_T, _, status, obj, _ = d.optimize(time_weight=w)
        T = d_T.cpu().numpy()
        assert np.all(status.cpu().numpy() == U.UAVQP_SOLVED)
        A = C_R[r] * dist ** 2
        T_star = ((2 * r - 1) * A / w) ** (1.0 / (2 * r))
        f_star = A / T_star ** (2 * r - 1) + w * T_star
        f_start = A + w
        assert np.max(np.abs(obj[:, 0] - f_start) / f_start) <= 1e-9
        assert np.all(obj[:, 1] <= obj[:, 0]) and np.all(obj[:, 1] >= f_star * (1.0 - 1e-9))
        sel = f_start > 1.5 * f_star
        gap = (obj[sel, 1] - f_star[sel]) / (f_start[sel] - f_star[sel])
        checked += int(sel.sum())
        worst_gap = max(worst_gap, gap.max())
        worst_T = max(worst_T, np.max(np.abs(T[sel] - T_star[sel]) / T_star[sel]))
        assert gap.max() <= 0.05, f"w = {w}: gap {gap.max():.3e}"
    print(f"r={r}: {checked} single-segment problems, worst gap {worst_gap:.3e}, worst |T - T*| / T* {worst_T:.3e}")
    assert checked >= 3 * n // 2


def test_optimiser_vs_scipy_lbfgsb_on_the_oracle(gpu_ctx, oracle):
    """>= 32 trajectories of 2 .. 6 segments whose waypoint spacing varies 8 x, from the reference's T = 1.0, w = 50, r = 3 and 4, half of them
    with non-zero boundary derivatives.  Reference: L-BFGS-B on the oracle's J*(T) + w sum T over the same box (run in log T: the same
    feasible set, the same objective).  OBJECTIVES are compared: gap = (f_lib - f_scipy) / (f_start - f_scipy) <= 0.05."""
    from scipy.optimize import minimize
    P = defaults()
    w, worst, ratios, count = 50.0, -1.0, [], 0
    rng = np.random.default_rng(2024)
    for r in (3, 4):
        n = 16
        Ms = rng.integers(2, 7, size=n)
        so = np.zeros(n + 1, dtype=np.int32)
        so[1:] = np.cumsum(Ms)
        wps, bc = [], np.zeros((n, 2, r - 1, 3))
        for t in range(n):
            M = int(Ms[t])
            steps = rng.choice([0.5, 2.0, 4.0], size=M)
            steps[0], steps[-1] = 0.5, 4.0
            dirs = rng.normal(size=(M, 3))
            wps.append(np.vstack([np.zeros(3), np.cumsum(dirs / np.linalg.norm(dirs, axis=1)[:, None] * steps[:, None], axis=0)]))
            if t % 2:
                bc[t] = rng.normal(size=(2, r - 1, 3))
        b = dict(r=r, seg_offsets=so, waypoints=np.vstack(wps), times=np.ones(int(so[-1])), bc=bc)
        d = Dev(gpu_ctx, b, False)
        _, _, status, obj, _ = d.optimize(time_weight=w)
        assert np.all(status.cpu().numpy() == U.UAVQP_SOLVED)
        for t in range(n):
            def f(u):
                T = np.exp(u)
                return sum(2.0 * oracle.cost(r, T, oracle.solve_exact(r, wps[t][:, ax], bc[t, 0, :, ax], bc[t, 1, :, ax], T)) for ax in range(3)) + w * T.sum()
            M = int(Ms[t])
            res = minimize(f, np.zeros(M), method="L-BFGS-B", bounds=[(math.log(P.t_min), math.log(P.t_max))] * M,
                           options=dict(maxiter=500, ftol=1e-13, gtol=1e-9))
            f_start, f_scipy = f(np.zeros(M)), float(res.fun)
            assert abs(obj[t, 0] - f_start) <= 1e-9 * f_start
            assert f_start > 1.5 * f_scipy, "the case has no decrease to speak of"
            gap = (obj[t, 1] - f_scipy) / (f_start - f_scipy)
            worst = max(worst, gap)
            ratios.append(f_start / f_scipy)
            count += 1
            assert gap <= 0.05, f"r={r} trajectory {t} (M={M}): gap {gap:.3e}"
    print(f"{count} multi-segment trajectories, f_start / f_scipy {min(ratios):.1f} .. {max(ratios):.1f}, worst gap {worst:.3e} "
          f"at max_iters = {P.max_iters}")
    assert count >= 32


def test_python_facade_optimize_time_and_get_cost(oracle):
    b = W.uniform_batch(2, 40, 6, 3, time_mode="reference")
    opt = U.TrajOptimizer(order=3)
    opt.setWaypoints(b["waypoints"].reshape(-1, 3), n_waypoints=7)
    opt.setTimeAllocation(b["times"])
    opt.setBoundary(b["bc"])
    assert opt.solve() is True
    cost0 = opt.getCost()
    ref, _ = oracle.solve_exact_batch(3, b["seg_offsets"], b["waypoints"], b["times"], b["bc"])
    want = oracle_costs(oracle, 3, np.asarray(b["seg_offsets"]), b["times"].ravel(), ref)
    assert np.max(np.abs(cost0 - want) / want) <= 1e-9
    assert opt.optimizeTime(time_weight=20.0) is True
    T = opt.getTimeAllocation()
    assert T.shape == (240,) and not np.array_equal(T, b["times"].ravel())
    assert np.all(opt.objective[:, 1] <= opt.objective[:, 0])
    assert np.max(np.abs(opt.objective[:, 0] - (cost0 + 20.0 * 6.0)) / opt.objective[:, 0]) <= 1e-12
    # getPolyCoeff stays valid: it is the solve at the stored allocation, and getCost is the cost of exactly that
    coef = opt.getPolyCoeff()
    cost1 = opt.getCost()
    assert np.max(np.abs(cost1 + 20.0 * T.reshape(40, 6).sum(axis=1) - opt.objective[:, 1]) / opt.objective[:, 1]) <= 1e-12
    assert opt.solve() is True
    assert np.array_equal(opt.getPolyCoeff(), coef)
    opt.setCorridor(b["waypoints"].reshape(-1, 3) - 0.1, b["waypoints"].reshape(-1, 3) + 0.1)
    with pytest.raises(ValueError):
        opt.optimizeTime(time_weight=20.0)


def test_cpp_facade_optimize_time():
    """Compiles tests/cpp/test_time_opt_facade.cpp against cpp/traj_optimizer.h and runs it on the GPU."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_time_opt_facade")
    pkg = os.path.join(ROOT, "uav_motion_planning_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++14", f"-I{pkg}/cpp", os.path.join(ROOT, "tests", "cpp", "test_time_opt_facade.cpp"),
                           f"-L{pkg}", "-luavqp", f"-Wl,-rpath,{pkg}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "optimizeTime" in out.stdout
