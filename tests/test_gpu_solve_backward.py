"""-m gpu: the backward pass of the batched solve (uavqp_solve_backward_device / _host, uav_motion_planning_amd.autograd) against the CPU oracle.

References (tests/test_solve_backward_contract.py pins them against the binary128 oracle): for grad_waypoints / grad_bc the dense KKT adjoint
on the oracle's matrices -- and, where that double-precision solve of the TEST is the limiting term, exact differences of oracle solves (c* is
linear in the waypoints and the boundary derivatives); for grad_times central differences of the binary128 minimiser under the project's
Richardson rule (the scheme's own error, h against h / 2, below 1e-5; the device within 10 x of it).  Tolerance for waypoints / bc: the project's
parity tolerance, 1e-9 relative to max|grad| of that array per trajectory.

Figures: docs/measurement_log.md, "Backward pass of the solve" (every test prints its worst case with -s).
Trajectories of more than 24 segments (25 to 96, every forward kernel, workspace records of interior knots): tests/test_gpu_long_gradients.py."""
import os
import subprocess

import numpy as np
import pytest

import uav_motion_planning_amd as U
from uav_motion_planning_amd import workloads as W

from test_solve_backward_contract import exact_linear_gradients, kkt_adjoint, random_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9


class Dev:
    """One batch on the device: solve and backward through the device-pointer entries."""

    def __init__(self, ctx, r, so, wp, T, bc, uniform):
        import torch
        self.torch, self.ctx, self.r = torch, ctx, r
        self.so = np.ascontiguousarray(so, dtype=np.int32)
        self.n = self.so.size - 1
        self.mmax = int(np.max(np.diff(self.so)))
        self.uni = self.mmax if uniform else 0
        self.total = int(self.so[-1])
        self.dev = torch.device("cuda", 0)
        self.wp = np.ascontiguousarray(wp, dtype=np.float64).reshape(-1, 3)
        self.T = np.ascontiguousarray(T, dtype=np.float64).ravel()
        self.bc = np.ascontiguousarray(bc, dtype=np.float64).reshape(self.n, 2, r - 1, 3)
        self.d_so = torch.from_numpy(self.so).to(self.dev)
        self.d_wp, self.d_T, self.d_bc = (torch.from_numpy(a).to(self.dev) for a in (self.wp, self.T, self.bc))

    def traj(self, b):
        s0, s1 = int(self.so[b]), int(self.so[b + 1])
        return s0, s1, self.wp[s0 + b:s1 + b + 1], self.bc[b], self.T[s0:s1]

    def solve(self, d_T=None):
        t = self.torch
        coeff = t.zeros(3 * 2 * self.r * self.total, dtype=t.float64, device=self.dev)
        status = t.zeros(self.n, dtype=t.int32, device=self.dev)
        t.cuda.synchronize()
        self.ctx.solve_batch_device(self.r, self.n, self.uni, self.mmax, self.d_so, self.d_wp, self.d_T if d_T is None else d_T, self.d_bc, coeff, status)
        self.ctx.synchronize()
        return coeff, status

    def backward(self, coeff, g, status=None, want=(True, True, True), d_T=None, fill=0.0):
        t = self.torch
        d_g = g if t.is_tensor(g) else t.from_numpy(np.ascontiguousarray(g, dtype=np.float64).ravel()).to(self.dev)
        g_t = t.full((self.total,), fill, dtype=t.float64, device=self.dev) if want[0] else None
        g_w = t.full((self.total + self.n, 3), fill, dtype=t.float64, device=self.dev) if want[1] else None
        g_b = t.full((self.n, 2, self.r - 1, 3), fill, dtype=t.float64, device=self.dev) if want[2] else None
        t.cuda.synchronize()
        self.ctx.solve_backward_device(self.r, self.n, self.uni, self.mmax, self.total, self.d_so, self.d_wp, self.d_T if d_T is None else d_T, self.d_bc,
                                       coeff, d_g, grad_times=g_t, grad_waypoints=g_w, grad_bc=g_b, status=status)
        self.ctx.synchronize()
        return g_t, g_w, g_b


def to_np(x):
    return None if x is None else x.cpu().numpy()


def hinge_gradient(r, so, T, coeff, v_lim, a_lim, K=8):
    """g = dPhi/dcoeff of Phi = sum over K samples per segment of relu(|v| - v_lim)^2 + relu(|a| - a_lim)^2: the realistic case (numpy)"""
    nc = 2 * r
    g = np.zeros_like(coeff)
    k = np.arange(nc)
    for b in range(so.size - 1):
        s0, s1 = int(so[b]), int(so[b + 1])
        M = s1 - s0
        c = coeff[3 * nc * s0:3 * nc * s1].reshape(3, M, nc)
        gb = np.zeros_like(c)
        for i in range(M):
            for tau in (np.arange(K) + 0.5) / K:
                t = tau * T[s0 + i]
                bv = np.where(k >= 1, k * t ** np.maximum(k - 1, 0), 0.0)
                ba = np.where(k >= 2, k * (k - 1) * t ** np.maximum(k - 2, 0), 0.0)
                for basis, lim in ((bv, v_lim), (ba, a_lim)):
                    x = c[:, i, :] @ basis
                    nx = np.linalg.norm(x)
                    if nx > lim:
                        gb[:, i, :] += 2.0 * (nx - lim) * (x / nx)[:, None] * basis[None, :]
        g[3 * nc * s0:3 * nc * s1] = gb.ravel()
    return g


def oracle_dcoeff_dT(oracle, r, wp, bc, T, h_rel):
    """central differences of the binary128 minimiser in every duration: [M][3 * M * 2r]"""
    out = []
    for i in range(T.size):
        e = np.zeros(T.size)
        e[i] = h_rel * T[i]
        cp = np.concatenate([oracle.solve_exact(r, wp[:, ax], bc[0, :, ax], bc[1, :, ax], T + e) for ax in range(3)])
        cm = np.concatenate([oracle.solve_exact(r, wp[:, ax], bc[0, :, ax], bc[1, :, ax], T - e) for ax in range(3)])
        out.append((cp - cm) / (2.0 * e[i]))
    return np.array(out)


def parity_batches(r):
    """uniform batches M in {1, 2, 3, 5, 8} in the shapes of the contract test, and one ragged batch with M from 1 to 24, non-zero bc"""
    out = []
    for M in (1, 2, 3, 5, 8):
        cases = [random_case(r, M, 9000 + 100 * r + 10 * M + j) for j in range(3)]
        so = (np.arange(len(cases) + 1) * M).astype(np.int32)
        out.append((f"uniform_M{M}", so, np.vstack([c[0] for c in cases]), np.concatenate([c[2] for c in cases]), np.array([c[1] for c in cases]), True))
    # workloads.py's kino-A*-like ragged batch (node duration 0.3 s), with one trajectory each at the two ends of the range appended
    parts = [W.ragged_batch(4, 10, r, m_lo=1, m_hi=24), W.ragged_batch(4, 1, r, m_lo=1, m_hi=1, seed=77), W.ragged_batch(4, 1, r, m_lo=24, m_hi=24, seed=78)]
    lens = np.concatenate([np.diff(p["seg_offsets"]) for p in parts])
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rng = np.random.default_rng(31 + r)
    bc = np.concatenate([p["bc"] for p in parts]) + rng.normal(size=(lens.size, 2, r - 1, 3))
    out.append(("ragged_M1to24", so, np.vstack([p["waypoints"] for p in parts]), np.concatenate([p["times"] for p in parts]), bc, False))
    return out


@pytest.mark.parametrize("r", [3, 4])
def test_parity_with_the_kkt_adjoint_and_the_oracle(gpu_ctx, oracle, r):
    worst = dict(w=0.0, b=0.0, t=0.0, rich=0.0)
    fallbacks = 0
    for name, so, wp, T, bc, uniform in parity_batches(r):
        d = Dev(gpu_ctx, r, so, wp, T, bc, uniform)
        coeff, st = d.solve()
        assert np.all(to_np(st) == U.UAVQP_SOLVED)
        c_np = to_np(coeff)
        rng = np.random.default_rng(5)
        fd = {}    # per trajectory: central differences of the binary128 minimiser at h and h / 2 (shared by the two g)
        for b in range(d.n):
            _, _, wp_b, bc_b, T_b = d.traj(b)
            fd[b] = (oracle_dcoeff_dT(oracle, r, wp_b, bc_b, T_b, 1e-4), oracle_dcoeff_dT(oracle, r, wp_b, bc_b, T_b, 0.5e-4))
        # (limits below what the trajectories reach, so that the hinge is active)
        for gname, g in (("normal", rng.normal(size=c_np.size)), ("hinge", hinge_gradient(r, d.so, d.T, c_np, 0.5, 1.0))):
            assert np.any(g != 0.0), f"{name}/{gname}: the hinge is not active"
            g_t, g_w, g_b = (to_np(x) for x in d.backward(coeff, g, status=st))
            for b in range(d.n):
                s0, s1, wp_b, bc_b, T_b = d.traj(b)
                M, nc = s1 - s0, 2 * r
                gb = g[3 * nc * s0:3 * nc * s1].reshape(3, M, nc)
                rT, rW, rB = kkt_adjoint(oracle, r, wp_b, bc_b, T_b, gb)
                dW, dB, dT = g_w[s0 + b:s1 + b + 1], g_b[b], g_t[s0:s1]
                ew = np.max(np.abs(dW - rW)) / np.max(np.abs(rW))
                eb = np.max(np.abs(dB - rB)) / np.max(np.abs(rB))
                if ew > TOL or eb > TOL:
                    # the test's own double-precision KKT solve may be the limiting term (it grows with M): exact oracle differences decide
                    fallbacks += 1
                    xW, xB = exact_linear_gradients(oracle, r, wp_b, bc_b, T_b, gb)
                    ew = np.max(np.abs(dW - xW)) / np.max(np.abs(xW))
                    eb = np.max(np.abs(dB - xB)) / np.max(np.abs(xB))
                    print(f"  {name}/{gname} trajectory {b} (M={M}): decided by exact oracle differences: waypoints {ew:.3e}, bc {eb:.3e}")
                worst["w"], worst["b"] = max(worst["w"], ew), max(worst["b"], eb)
                assert ew <= TOL, f"{name}/{gname} trajectory {b} (M={M}): grad_waypoints {ew:.3e}"
                assert eb <= TOL, f"{name}/{gname} trajectory {b} (M={M}): grad_bc {eb:.3e}"
                # durations: binary128 central differences, Richardson rule
                f1, f2 = fd[b][0] @ gb.ravel(), fd[b][1] @ gb.ravel()
                scale = np.max(np.abs(f2))
                rich = np.max(np.abs(f1 - f2)) / scale
                et = np.max(np.abs(dT - f2)) / scale
                worst["t"], worst["rich"] = max(worst["t"], et), max(worst["rich"], rich)
                assert rich < 1e-5, f"{name}/{gname} trajectory {b}: the finite-difference step is badly chosen ({rich:.3e})"
                assert et <= 10.0 * rich, f"{name}/{gname} trajectory {b} (M={M}): grad_times {et:.3e} vs Richardson {rich:.3e}"
    print(f"r={r}: worst rel err waypoints {worst['w']:.3e}, bc {worst['b']:.3e}; times |device - fd| {worst['t']:.3e} at a Richardson estimate of "
          f"{worst['rich']:.3e}; {fallbacks} trajectories decided by exact oracle differences")


@pytest.mark.parametrize("r,uniform", [(4, True), (3, False)])
def test_tie_to_the_closed_form_time_gradient(gpu_ctx, oracle, r, uniform):
    """g = 2 P c*: Phi = c' P c.  Total derivative = through-c* part (this entry) + explicit part c' dP/dT_i c = sum over axes (p^(r)(T_i))^2
    = what uavqp_cost_time_gradient_device returns.  The two parts cancel to a large extent (the through part alone is -2 x the explicit one
    for a single rest-to-rest segment), so the comparison is relative to the larger of the terms that are summed, per trajectory, at the 1e-9
    of that kernel's cost / homogeneity tests."""
    import math
    b = W.uniform_batch(2, 64, 8, r, time_mode="distance") if uniform else W.ragged_batch(4, 64, r, m_lo=1, m_hi=24)
    rng = np.random.default_rng(3)
    bc = np.array(b["bc"]) + rng.uniform(-1.0, 1.0, size=np.shape(b["bc"]))
    d = Dev(gpu_ctx, r, b["seg_offsets"], b["waypoints"], b["times"], bc, uniform)
    coeff, st = d.solve()
    assert np.all(to_np(st) == U.UAVQP_SOLVED)
    c_np, nc = to_np(coeff), 2 * r
    g, explicit = np.zeros_like(c_np), np.zeros(d.total)
    for t in range(d.n):
        s0, s1, _, _, T_t = d.traj(t)
        P, _ = oracle.assemble(r, T_t)
        c = c_np[3 * nc * s0:3 * nc * s1].reshape(3, -1)
        g[3 * nc * s0:3 * nc * s1] = (2.0 * c @ P).ravel()
        k = np.arange(r, nc)
        fall = np.array([math.factorial(int(j)) / math.factorial(int(j) - r) for j in k])
        cs = c.reshape(3, s1 - s0, nc)
        pr = np.einsum("aik,ik->ai", cs[:, :, r:] * fall, T_t[:, None] ** (k - r)[None, :])   # p^(r)(T_i)
        explicit[s0:s1] = np.sum(pr ** 2, axis=0)
    g_t, _, _ = d.backward(coeff, g, status=st)
    t = d.torch
    closed = t.zeros(d.total, dtype=t.float64, device=d.dev)
    gpu_ctx.cost_time_gradient_device(r, d.n, d.uni, d.d_so, d.d_T, coeff, None, closed)
    gpu_ctx.synchronize()
    total, closed = to_np(g_t) + explicit, to_np(closed)
    worst = 0.0
    for tr in range(d.n):
        s0, s1 = int(d.so[tr]), int(d.so[tr + 1])
        scale = max(np.max(np.abs(closed[s0:s1])), np.max(explicit[s0:s1]), np.max(np.abs(to_np(g_t)[s0:s1])))
        worst = max(worst, np.max(np.abs(total[s0:s1] - closed[s0:s1])) / scale)
    print(f"r={r} {'uniform' if uniform else 'ragged'}: max |through + explicit - closed form| / max term = {worst:.3e}")
    assert worst <= 1e-9


def test_invalid_unsolved_null_outputs_bitwise_and_host_entry(gpu_ctx):
    r = 4
    b = W.ragged_batch(4, 200, r, m_lo=1, m_hi=12)
    rng = np.random.default_rng(11)
    bc = np.array(b["bc"]) + rng.uniform(-1.0, 1.0, size=np.shape(b["bc"]))
    T = np.array(b["times"], dtype=np.float64)
    so = np.asarray(b["seg_offsets"])
    bad_T, bad_nan, bad_st = 7, 50, 120
    T_bad = T.copy()
    T_bad[so[bad_T] + (so[bad_T + 1] - so[bad_T]) // 2] = -1.0
    T_bad[so[bad_nan]] = np.nan
    good = Dev(gpu_ctx, r, so, b["waypoints"], T, bc, False)
    d = Dev(gpu_ctx, r, so, b["waypoints"], T_bad, bc, False)
    coeff, st = d.solve()
    st_np = to_np(st)
    assert st_np[bad_T] == U.UAVQP_INVALID_INPUT and st_np[bad_nan] == U.UAVQP_INVALID_INPUT
    st2 = st.clone()
    st2[bad_st] = U.UAVQP_NON_FINITE          # a trajectory whose passed status says "not solved"
    g = rng.normal(size=coeff.numel())
    # outputs pre-filled with NaN: every element must be written
    out = [to_np(x) for x in d.backward(coeff, g, status=st2, fill=float("nan"))]
    assert all(np.all(np.isfinite(x)) for x in out), "an output element was left unwritten"
    g_t, g_w, g_b = out
    # neighbours unaffected: the same numbers as a batch without the bad entries
    c_good, st_good = good.solve()
    ref = [to_np(x) for x in good.backward(c_good, g, status=st_good)]
    for tr in range(d.n):
        s0, s1 = int(so[tr]), int(so[tr + 1])
        mine = (g_t[s0:s1], g_w[s0 + tr:s1 + tr + 1], g_b[tr])
        if tr in (bad_T, bad_nan, bad_st):
            assert all(np.all(x == 0.0) for x in mine), f"trajectory {tr} must carry zero gradients"
        else:
            theirs = (ref[0][s0:s1], ref[1][s0 + tr:s1 + tr + 1], ref[2][tr])
            assert all(np.array_equal(x, y) for x, y in zip(mine, theirs)), f"trajectory {tr} was affected by an invalid neighbour"
    # without a status array only the durations decide
    g_t3, _, _ = d.backward(coeff, g, status=None)
    s0, s1 = int(so[bad_st]), int(so[bad_st + 1])
    assert np.array_equal(to_np(g_t3)[s0:s1], ref[0][s0:s1]) and np.all(to_np(g_t3)[int(so[bad_T]):int(so[bad_T + 1])] == 0.0)
    # each output may be NULL, the others are unchanged to the bit; all NULL is a no-op
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False)):
        got = d.backward(coeff, g, status=st2, want=want)
        for have, x, y in zip(want, got, out):
            assert (x is None) if not have else np.array_equal(to_np(x), y)
    assert d.backward(coeff, g, status=st2, want=(False, False, False)) == (None, None, None)
    # two runs: the same bytes
    again = [to_np(x) for x in d.backward(coeff, g, status=st2)]
    assert all(np.array_equal(x, y) for x, y in zip(again, out))
    # host entry = device entry, bitwise
    host = gpu_ctx.solve_backward_host(r, so, b["waypoints"], T_bad, bc, to_np(coeff), g, status=to_np(st2))
    assert all(np.array_equal(np.asarray(x).reshape(y.shape), y) for x, y in zip(host, out))
    # uniform batches take the same kernel: a uniform batch given as CSR gives the same bytes
    bu = W.uniform_batch(2, 130, 5, r, time_mode="distance")
    du, dr = Dev(gpu_ctx, r, bu["seg_offsets"], bu["waypoints"], bu["times"], bu["bc"], True), Dev(gpu_ctx, r, bu["seg_offsets"], bu["waypoints"], bu["times"], bu["bc"], False)
    cu, su = du.solve()
    gu = rng.normal(size=cu.numel())
    assert all(np.array_equal(to_np(x), to_np(y)) for x, y in zip(du.backward(cu, gu, status=su), dr.backward(cu, gu, status=su)))


def test_grid_stride_rounds_equal_separate_launches(gpu_ctx):
    """Above 64 x 2 x (number of CUs) trajectories the kernel strides over the batch and a lane re-uses its workspace record round after
    round: 40000 trajectories in one launch give the bytes of the same data run as two launches of 20000 (single round each)."""
    r, n, M = 3, 40000, 1
    b = W.uniform_batch(1, n, M, r, time_mode="distance")
    rng = np.random.default_rng(21)
    bc = np.array(b["bc"]) + rng.uniform(-1.0, 1.0, size=np.shape(b["bc"]))
    g = rng.normal(size=3 * 2 * r * n * M)
    whole = Dev(gpu_ctx, r, b["seg_offsets"], b["waypoints"], b["times"], bc, True)
    coeff, st = whole.solve()
    assert np.all(to_np(st) == U.UAVQP_SOLVED)
    got = [to_np(x) for x in whole.backward(coeff, g, status=st)]
    h, per = n // 2, 3 * 2 * r * M
    for lo in (0, h):
        part = Dev(gpu_ctx, r, b["seg_offsets"][:h + 1], b["waypoints"][lo:lo + h], b["times"][lo:lo + h], bc[lo:lo + h], True)
        c_p, st_p = coeff[per * lo:per * (lo + h)].clone(), st[lo:lo + h].clone()
        ref = [to_np(x) for x in part.backward(c_p, g[per * lo:per * (lo + h)], status=st_p)]
        assert np.array_equal(got[0][M * lo:M * (lo + h)], ref[0])
        assert np.array_equal(got[1][(M + 1) * lo:(M + 1) * (lo + h)], ref[1])
        assert np.array_equal(got[2][lo:lo + h], ref[2])
    assert np.all(np.isfinite(got[0])) and np.any(got[0] != 0.0)


def test_error_codes(gpu_ctx):
    r = 3
    b = W.uniform_batch(2, 8, 4, r, time_mode="distance")
    d = Dev(gpu_ctx, r, b["seg_offsets"], b["waypoints"], b["times"], b["bc"], True)
    coeff, st = d.solve()
    t = d.torch
    g = t.ones_like(coeff)
    g_t = t.zeros(d.total, dtype=t.float64, device=d.dev)
    ok = dict(r=r, n_traj=d.n, uniform_segments=d.uni, max_segments=d.mmax, total_segments=d.total, seg_offsets=d.d_so, waypoints=d.d_wp, times=d.d_T,
              bc=d.d_bc, coeff=coeff, grad_coeff=g, grad_times=g_t)
    gpu_ctx.solve_backward_device(**ok)
    gpu_ctx.synchronize()
    for bad in (dict(r=5), dict(n_traj=-1), dict(uniform_segments=-1), dict(total_segments=-1), dict(total_segments=d.total + 1), dict(waypoints=None),
                dict(times=None), dict(bc=None), dict(coeff=None), dict(grad_coeff=None), dict(uniform_segments=0, seg_offsets=None),
                dict(uniform_segments=0, max_segments=0)):
        with pytest.raises(U.UavqpError):
            gpu_ctx.solve_backward_device(**dict(ok, **bad))
    gpu_ctx.solve_backward_device(**dict(ok, n_traj=0, total_segments=0))     # an empty batch is fine
    gpu_ctx.solve_backward_device(**dict(ok, grad_times=None, coeff=None))    # nothing asked for: nothing checked, nothing done
    # host entry: ragged without offsets, and a NULL input
    from uav_motion_planning_amd import _lib
    from uav_motion_planning_amd.traj_optimizer import _ptr
    h = [np.ascontiguousarray(x, dtype=np.float64) for x in (b["waypoints"], b["times"], b["bc"], to_np(coeff), to_np(g))]
    out = np.zeros(d.total)
    host = _lib.lib().uavqp_solve_backward_host
    assert host(gpu_ctx._h, r, d.n, 0, d.mmax, None, _ptr(h[0]), _ptr(h[1]), _ptr(h[2]), _ptr(h[3]), None, _ptr(h[4]), _ptr(out), None, None) == _lib.UAVQP_ERR_INVALID_ARG
    assert host(gpu_ctx._h, r, d.n, d.uni, d.mmax, None, _ptr(h[0]), _ptr(h[1]), _ptr(h[2]), None, None, _ptr(h[4]), _ptr(out), None, None) == _lib.UAVQP_ERR_INVALID_ARG
    assert host(gpu_ctx._h, r, d.n, d.uni, d.mmax, None, _ptr(h[0]), _ptr(h[1]), _ptr(h[2]), _ptr(h[3]), None, _ptr(h[4]), _ptr(out), None, None) == _lib.UAVQP_OK
    assert np.array_equal(out, to_np(g_t))
    gpu_ctx.synchronize()


def test_guard_bands_around_the_outputs(gpu_ctx):
    """pattern of tests/test_gpu_guard_bands.py: every array of the call inside one allocation with sentinel bands, edge-case shapes."""
    from test_gpu_guard_bands import Arena, _both_fills
    for r in (3, 4):
        rng = np.random.default_rng(100 + r)
        lens = np.array([1, 3, 0, 7, 1, 12, 2] + list(rng.integers(1, 9, size=70)))     # a zero-segment trajectory, lanes without a problem
        so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        n, total = lens.size, int(so[-1])
        wp = rng.normal(size=(total + n, 3)).cumsum(axis=0)
        T = rng.uniform(0.5, 2.0, size=total)
        T[int(so[5]) + 3] = 0.0                                                           # an invalid duration
        bc = rng.normal(size=(n, 2, r - 1, 3))

        def run_backward(ar, r=r, so=so, wp=wp, T=T, bc=bc, n=n, total=total):
            d_so, d_wp, d_T, d_bc = ar.put(so), ar.put(wp), ar.put(T), ar.put(bc)
            coeff, st = ar.out(3 * 2 * r * total), ar.out(n, np.int32)
            gpu_ctx.solve_batch_device(r, n, 0, 12, d_so, d_wp, d_T, d_bc, coeff, st)
            g = ar.put(np.random.default_rng(1).normal(size=3 * 2 * r * total))
            g_t, g_w, g_b = ar.out(total, misalign=8), ar.out((total + n, 3)), ar.out((n, 2, r - 1, 3), misalign=8)
            gpu_ctx.solve_backward_device(r, n, 0, 12, total, d_so, d_wp, d_T, d_bc, coeff, g, grad_times=g_t, grad_waypoints=g_w, grad_bc=g_b, status=st)
            gpu_ctx.synchronize()
            return dict(g_t=g_t, g_w=g_w, g_b=g_b)
        res = _both_fills(run_backward)
        assert np.any(res["g_t"] != 0.0)


def _torch_batch(b, r, dev, rng=None):
    import torch
    wp = torch.tensor(np.asarray(b["waypoints"]).reshape(-1, 3), dtype=torch.float64, device=dev)
    T = torch.tensor(np.asarray(b["times"]).ravel(), dtype=torch.float64, device=dev)
    bc = np.array(b["bc"], dtype=np.float64)
    if rng is not None:
        bc = bc + rng.uniform(-1.0, 1.0, size=bc.shape)
    return wp, T, torch.tensor(bc, dtype=torch.float64, device=dev)


def test_autograd_reproduces_the_c_abi_bitwise(gpu_ctx):
    import torch
    from uav_motion_planning_amd.autograd import solve_batch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(8)
    for r, b, uniform in ((4, W.uniform_batch(2, 300, 8, 4, time_mode="distance"), 8), (3, W.ragged_batch(4, 300, 3, m_lo=1, m_hi=24), 0)):
        wp, T, bc = _torch_batch(b, r, dev, rng)
        so = torch.from_numpy(np.ascontiguousarray(b["seg_offsets"], dtype=np.int32)).to(dev)
        d = Dev(gpu_ctx, r, b["seg_offsets"], wp.cpu().numpy(), T.cpu().numpy(), bc.cpu().numpy(), uniform > 0)
        coeff_ref, st = d.solve()
        g = torch.from_numpy(rng.normal(size=coeff_ref.numel())).to(dev)
        ref = d.backward(coeff_ref, g, status=st)
        for t_ in (wp, T, bc):
            t_.requires_grad_(True)
        coeff = solve_batch(gpu_ctx, r, wp, T, bc, seg_offsets=None if uniform else so, uniform_segments=uniform, check_status=True)
        assert torch.equal(coeff.detach(), coeff_ref)
        (coeff * g).sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(T.grad, ref[0]) and torch.equal(wp.grad, ref[1]) and torch.equal(bc.grad, ref[2])
        # only what needs_input_grad asks for
        T2 = T.detach().clone().requires_grad_(True)
        c2 = solve_batch(gpu_ctx, r, wp.detach(), T2, bc.detach(), seg_offsets=None if uniform else so, uniform_segments=uniform)
        (c2 * g).sum().backward()
        assert torch.equal(T2.grad, ref[0])
    gpu_ctx.set_stream(None)
    # an unsolved trajectory: zero gradient by default, an error on request
    T_bad = T.detach().clone()
    T_bad[3] = -1.0
    T_bad.requires_grad_(True)
    c3, st3 = solve_batch(gpu_ctx, r, wp.detach(), T_bad, bc.detach(), seg_offsets=so, return_status=True)
    (c3 * g).sum().backward()
    tr = int(np.searchsorted(np.asarray(b["seg_offsets"]), 3, side="right") - 1)
    s0, s1 = int(b["seg_offsets"][tr]), int(b["seg_offsets"][tr + 1])
    assert int(st3[tr]) == U.UAVQP_INVALID_INPUT and bool((T_bad.grad[s0:s1] == 0.0).all()) and bool((T_bad.grad[s1:] != 0.0).any())
    with pytest.raises(U.UavqpError):
        solve_batch(gpu_ctx, r, wp.detach(), T_bad.detach(), bc.detach(), seg_offsets=so, check_status=True)
    gpu_ctx.set_stream(None)


def test_autograd_directional_derivative_through_the_device_forward(gpu_ctx):
    """(Phi(x + eps d) - Phi(x - eps d)) / 2 eps against grad . d, x = (times, waypoints, bc) jointly, Phi a smooth non-linear function of the
    coefficients, everything through the DEVICE forward; the project's Richardson rule (eps against eps / 2)."""
    import torch
    from uav_motion_planning_amd.autograd import solve_batch
    dev = torch.device("cuda", 0)
    for r, M in ((3, 5), (4, 8)):
        rng = np.random.default_rng(40 + r)
        b = W.uniform_batch(2, 16, M, r, time_mode="distance")
        wp, T, bc = _torch_batch(b, r, dev, rng)
        g = torch.from_numpy(rng.normal(size=3 * 2 * r * T.numel())).to(dev)

        def phi(wp_, T_, bc_):
            c = solve_batch(gpu_ctx, r, wp_, T_, bc_, uniform_segments=M, check_status=True)
            return (c * g).sum() + 0.5e-3 * (c * c).sum() + (T_ * T_).sum()      # (the last term: an explicit dependence on the durations)
        x = [t_.clone().requires_grad_(True) for t_ in (wp, T, bc)]
        phi(*x).backward()
        dirs = [torch.from_numpy(rng.normal(size=tuple(t_.shape))).to(dev) for t_ in x]
        dirs[1] = dirs[1] * T * 0.3           # durations move relative to their size
        slope = sum(float((t_.grad * d_).sum()) for t_, d_ in zip(x, dirs))

        def fd(eps):
            with torch.no_grad():
                hi = phi(*[t_.detach() + eps * d_ for t_, d_ in zip(x, dirs)])
                lo = phi(*[t_.detach() - eps * d_ for t_, d_ in zip(x, dirs)])
            return float(hi - lo) / (2.0 * eps)
        f1, f2 = fd(1e-4), fd(0.5e-4)
        rich, err = abs(f1 - f2) / abs(slope), abs(f2 - slope) / abs(slope)
        print(f"r={r} M={M}: directional derivative {slope:.9e}, |fd - grad.d| / |grad.d| = {err:.3e}, Richardson estimate {rich:.3e}")
        assert rich < 1e-5
        assert err <= 10.0 * rich
    gpu_ctx.set_stream(None)


def test_autograd_end_to_end_velocity_limit_descent(gpu_ctx):
    """4096 x 8, r = 4: plain gradient steps on u = log T for  L_b = sum over samples of relu(|v| - V_LIM)^2 + W_TIME * sum T  per trajectory,
    step length per trajectory, halved when a trial does not lower L_b and doubled when it does (trajectories are independent problems).
    A wrong sign or scale of the gradient stalls at step one: every trajectory with a gradient must accept a step, every accepted step lowers
    its loss (the step rule), and after STEPS steps the total loss and the number of limit-violating samples are strictly below the start."""
    import torch
    from uav_motion_planning_amd.autograd import solve_batch
    V_LIM, W_TIME, STEPS, K = 2.5, 0.01, 12, 8
    r, n, M = 4, 4096, 8
    dev = torch.device("cuda", 0)
    b = W.uniform_batch(2, n, M, r, time_mode="distance")     # T_i = |dp| / 2 m/s: mean speed 2 m/s, peaks above the limit
    wp, T0, bc = _torch_batch(b, r, dev)
    tau = (torch.arange(K, dtype=torch.float64, device=dev) + 0.5) / K
    k = torch.arange(1, 2 * r, dtype=torch.float64, device=dev)

    def losses(u):
        T = torch.exp(u)
        c = solve_batch(gpu_ctx, r, wp, T, bc, uniform_segments=M).view(n, 3, M, 2 * r)
        t = T.view(n, 1, M, 1, 1) * tau.view(1, 1, 1, K, 1)                                  # [n, 1, M, K, 1]
        v = (c[:, :, :, None, 1:] * k * t ** (k - 1.0)).sum(-1)                              # [n, 3, M, K]
        speed = torch.sqrt((v * v).sum(1) + 1e-30)
        over = torch.relu(speed - V_LIM)
        return (over * over).sum((1, 2)) + W_TIME * T.view(n, M).sum(1), int((speed > V_LIM).sum())

    u = torch.log(T0).requires_grad_(True)
    L, viol0 = losses(u)
    L0 = L.detach().clone()
    assert viol0 > 0, "the start must violate the limit"
    L.sum().backward()
    grad = u.grad.view(n, M).clone()
    alpha = 0.1 / grad.abs().amax(1).clamp_min(1e-300)      # the first trial moves the most sensitive duration by 10 %
    accepted = torch.zeros(n, dtype=torch.int64, device=dev)
    u_best, L_best = u.detach().view(n, M).clone(), L0.clone()
    for _ in range(STEPS):
        trial = (u_best - alpha[:, None] * grad).reshape(-1).requires_grad_(True)
        L_t, _ = losses(trial)
        L_t.sum().backward()
        better = L_t.detach() < L_best
        assert bool((L_t.detach()[better] < L_best[better]).all())    # (true by the definition of `better`: the step rule itself, not a check;
        #  what can fail is below: every trajectory accepts a step, the loss and the violation count end lower)
        u_best = torch.where(better[:, None], trial.detach().view(n, M), u_best)
        grad = torch.where(better[:, None], trial.grad.view(n, M), grad)
        L_best = torch.where(better, L_t.detach(), L_best)
        accepted += better.long()
        alpha = torch.where(better, alpha * 2.0, alpha * 0.5)
    with torch.no_grad():
        L1, viol1 = losses(u_best.reshape(-1))
    gpu_ctx.set_stream(None)
    print(f"velocity-limit descent, {n} x {M}, r = {r}, v_lim {V_LIM} m/s, w {W_TIME}, {STEPS} steps: total loss {float(L0.sum()):.6e} -> {float(L1.sum()):.6e}, "
          f"violating samples {viol0} -> {viol1} of {n * M * K}, accepted steps per trajectory min / median / max "
          f"{int(accepted.min())} / {int(accepted.median())} / {int(accepted.max())}")
    assert bool((L1 <= L0).all())
    assert int(accepted.min()) >= 1, "a trajectory never accepted a step: wrong gradient sign or scale"
    assert float(L1.sum()) < float(L0.sum()) and viol1 < viol0


def test_python_facade_backward(oracle):
    r = 3
    b = W.uniform_batch(2, 6, 5, r, time_mode="distance")
    opt = U.TrajOptimizer(order=r)
    opt.setWaypoints(b["waypoints"].reshape(-1, 3), n_waypoints=6)
    opt.setTimeAllocation(b["times"])
    opt.setBoundary(b["bc"])
    with pytest.raises(U.UavqpError):
        opt.backward(np.zeros(3 * 6 * 30))
    assert opt.solve() is True
    g = np.random.default_rng(2).normal(size=opt.getPolyCoeff().size)
    g_t, g_w, g_b = opt.backward(g)
    assert g_t.shape == (30,) and g_w.shape == (36, 3) and g_b.shape == (6, 2, 2, 3)
    for t in range(6):
        rT, rW, rB = kkt_adjoint(oracle, r, b["waypoints"][t], b["bc"][t], b["times"][t], g[90 * t:90 * (t + 1)].reshape(3, 5, 6))
        assert np.max(np.abs(g_w[6 * t:6 * t + 6] - rW)) <= TOL * np.max(np.abs(rW))
        assert np.max(np.abs(g_b[t] - rB)) <= TOL * np.max(np.abs(rB))
        assert np.max(np.abs(g_t[5 * t:5 * t + 5] - rT)) <= TOL * np.max(np.abs(rT))
    opt.setCorridor(b["waypoints"].reshape(-1, 3) - 0.1, b["waypoints"].reshape(-1, 3) + 0.1)
    with pytest.raises(ValueError):
        opt.backward(g)


def test_cpp_facade_backward():
    """Compiles tests/cpp/test_solve_backward_facade.cpp against cpp/traj_optimizer.h and runs it on the GPU."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_solve_backward_facade")
    pkg = os.path.join(ROOT, "uav_motion_planning_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++14", f"-I{pkg}/cpp", os.path.join(ROOT, "tests", "cpp", "test_solve_backward_facade.cpp"),
                           f"-L{pkg}", "-luavqp", f"-Wl,-rpath,{pkg}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "backward" in out.stdout
