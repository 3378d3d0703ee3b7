"""A designed reference of the joint waypoint / duration optimiser (include/uavqp.h: uavqp_flight_penalty_device,
uavqp_spacetime_optimize_device), numpy only, written from the header text and not from the kernels.  Built on
tests/waypoint_opt_reference.py (scene, cases, uniform_cases, uniform11_cases, split), tests/limit_penalty_reference.py and
tests/esdf_reference.py (the two longdouble penalties).  Shared by tests/test_spacetime_contract.py (CPU), tests/test_gpu_spacetime.py and
tools/spacetime_convergence.py.

  Problem      one trajectory: f(p, T) = smooth_weight J + time_weight sum T + Phi_lim + Phi_clr on the oracle's exact solve, and its full
               gradient in (p, T).  The gradient does NOT use the closed forms the kernels use (dJ/dp from the leading coefficients,
               dJ/dT = -H): it differentiates the KKT system of the equality-constrained QP,
                   [2 P(T)  A(T)'] [c  ]   [0   ]
                   [A(T)    0    ] [lam] = [b(p)]
               by ONE adjoint solve K y = (dF/dc, 0) per axis with F = smooth_weight c' P c + Phi: the part of dF/dp_k through the minimiser
               is y_lam . db/dp_k, that of dF/dT_i is -y' (dK/dT_i) (c, lam); the explicit parts are smooth_weight c' (dP/dT_i) c, the
               penalties' own explicit time gradients and time_weight.  Every entry of P and A is a monomial in ONE duration, so dK/dT_i comes
               from the oracle's assembly itself: the exponent of an entry is log2 of its ratio at 2 T and at T (checked to be an integer).
  iterate()    the projected-gradient / Armijo iteration of the header, one trial per step, f after every trial
  lbfgsb()     scipy's L-BFGS-B on the same f from the same start in (p, log T), the box and log t_min / log t_max as bounds

Test parameters.  LIMITS_OF[r]: chosen on the CPU so that at scipy's optimum WITHOUT the limit penalty (weight_v = weight_a = 0) at least
half of the trajectories have a sampled peak above a limit -- in fact all of them, and by a margin: v_max and a_max are 0.7 x the median
of those peaks (tools/spacetime_convergence.py --limits on the seed-1 batches: r = 3: 2.39 m/s, 2.20 m/s^2; r = 4: 1.95 m/s, 1.43
m/s^2), rounded down to one decimal.  0.7 x the unconstrained peak is the setting for which include/uavqp.h states what a soft penalty
of weight 1e3 leaves (3 to 12 per cent above the limit): limits AT the median would put the unpenalised peaks inside that band, where a
penalised and an unpenalised result cannot be told apart.  tests/test_spacetime_contract.py asserts on the recorded optima that at least
half exceed a limit.
SEEDS: tools/spacetime_convergence.py --seed-search, the first seed from 1 per r for which EVERY trajectory of the ragged batch (seed)
and of the uniform batch (100 + seed) has
  * f_start > 1.5 f_scipy, and outside == 0 at the start, at scipy's optimum and at the transcription's result.  "The transcription's
    result" is that after FEASIBILITY_ITERS = 256 trials, the longest run of the study, NOT after the default max_iters: the default is
    chosen from the gaps on these very batches, and a seed rule that referred to it would have no fixed point (at 256 trials the gaps
    give 32, at 32 trials other seeds);
  * at the transcription's result a smaller peak, in every component in which scipy's optimum with both limit weights zero exceeds the
    limit, than at that optimum;
  * at the transcription's result a larger smallest distance than at scipy's optimum with clearance weight zero, wherever that optimum
    comes closer than d_safe (trajectories with an interior waypoint: one segment has nothing to move sideways);
  * the same two comparisons against the transcription's OWN runs with those weights zeroed, which is what
    tests/test_gpu_spacetime.py then asserts of the device;
and at least half of the trajectories of each batch take part in each comparison."""
import math

import numpy as np

import esdf_reference as E
import limit_penalty_reference as L
import waypoint_opt_reference as W

LD = np.longdouble
CLEARANCE = dict(W.CLEARANCE)
LIMITS_OF = {3: dict(samples_per_seg=8, v_max=1.6, a_max=1.5, weight_v=1e3, weight_a=1e3),
             4: dict(samples_per_seg=8, v_max=1.3, a_max=0.9, weight_v=1e3, weight_a=1e3)}
PARAMS = dict(smooth_weight=1.0, time_weight=50.0, t_min=1e-2, t_max=1e2, max_move=1.0, initial_step_move=0.1, initial_step_log=0.1,
              armijo_c=1e-4, shrink=0.5, grow=2.0)
SEEDS = {3: 24, 4: 3}
STEPS = (32, 64, 128, 256)
FEASIBILITY_ITERS = STEPS[-1]   # the trial count of the feasibility comparisons: fixed, so that seeds and default do not depend on each other
# The worst fraction of scipy's decrease the transcription leaves on cases(r) and uniform_cases(r), r = 3 and 4, after the library's default
# max_iters (tools/spacetime_convergence.py; DESIGN.md section 5.20 has the whole table), and the trajectory it is attained at.
DEFAULT_MAX_ITERS = 32
GAP_AT_DEFAULT = 1.997e-2
GAP_CASE = (3, "ragged", 9)

scene, split = W.scene, W.split


def cases(r, seed=None):
    return W.cases(r, seed=SEEDS[r] if seed is None else seed)


def uniform_cases(r, seed=None):
    return W.cases(r, seed=100 + (SEEDS[r] if seed is None else seed), Ms=[W.UNIFORM_M] * W.UNIFORM_N, ragged_times=False)


def uniform11_cases(r):
    return W.cases(r, seed=200 + SEEDS[r], Ms=[11] * 4, ragged_times=True)


def batch_of(r, kind):
    return dict(ragged=cases, uniform=uniform_cases, uniform11=uniform11_cases)[kind](r)


def clamp_times(T, **params):
    """The projection of the durations the optimiser starts with (all positive and finite: into [t_min, t_max])."""
    P = dict(PARAMS, **params)
    T = np.asarray(T, dtype=np.float64)
    return np.minimum(np.maximum(T, P["t_min"]), P["t_max"]) if np.all((T > 0) & np.isfinite(T)) else T.copy()


class Problem:
    """f(p, T) of one trajectory on the oracle's solve; p [M + 1][3] (the end rows are never moved), T [M]."""

    def __init__(self, oracle, r, wp, T, bc, limits=None, clearance=None, smooth_weight=PARAMS["smooth_weight"],
                 time_weight=PARAMS["time_weight"], sc=None):
        self.o, self.r = oracle, r
        self.bc = np.asarray(bc, dtype=np.float64)
        self.start_p = np.array(wp, dtype=np.float64)
        self.start_T = np.array(T, dtype=np.float64)
        self.M = self.start_T.size
        self.lp = dict(LIMITS_OF[r], **(limits or {}))
        self.cp = dict(CLEARANCE, **(clearance or {}))
        self.ws, self.wt = float(smooth_weight), float(time_weight)
        self.sc = scene() if sc is None else sc
        self.evals = 0

    # ---- f
    def coeff(self, p, T):
        """[3][M][2r]: the oracle's exact minimiser per axis"""
        return np.array([self.o.solve_exact(self.r, p[:, ax], self.bc[0, :, ax], self.bc[1, :, ax], T) for ax in range(3)]).reshape(3, self.M, 2 * self.r)

    def cost(self, c, T):
        return sum(2.0 * self.o.cost(self.r, T, c[ax].ravel()) for ax in range(3))

    def penalties(self, c, T):
        """-> (limit penalty dict, clearance penalty dict) of tests/limit_penalty_reference.py / tests/esdf_reference.py"""
        s = self.sc
        lim = L.penalty(self.r, [0, self.M], T, c.ravel(), **self.lp)
        clr = E.penalty(self.r, [0, self.M], T, c.ravel(), s["dist"], s["origin"], s["res"], s["max_dist"], **self.cp)
        return lim, clr

    def parts(self, p, T):
        """-> dict f, J, phi, lim, clr, c at (p, T)"""
        self.evals += 1
        c = self.coeff(p, T)
        J = self.cost(c, T)
        lim, clr = self.penalties(c, T)
        phi = float(lim["phi"][0] + clr["phi"][0])
        return dict(f=self.ws * J + self.wt * float(np.sum(T)) + phi, J=J, phi=phi, lim=lim, clr=clr, c=c,
                    peak=np.asarray(lim["peak"][0], dtype=np.float64), min_dist=float(clr["min_dist"][0]), outside=int(clr["outside"][0]))

    def f(self, p, T):
        return self.parts(p, T)["f"]

    # ---- gradient
    def _kkt(self, T):
        """-> (K, n, B [m][M + 1] = db/dp, dK [M] list of (dP_i, dA_i))"""
        r, M = self.r, self.M
        P, A = self.o.assemble(r, T)
        P2, A2 = self.o.assemble(r, 2.0 * np.asarray(T))
        n, m = P.shape[0], A.shape[0]
        K = np.zeros((n + m, n + m))
        K[:n, :n] = 2.0 * P
        K[:n, n:] = A.T
        K[n:, :n] = A
        z = np.zeros(r - 1)
        B = np.column_stack([self.o.bounds(r, np.eye(M + 1)[k], z, z)[0] for k in range(M + 1)])
        dK = []
        with np.errstate(divide="ignore", invalid="ignore"):
            eP = np.where(P != 0.0, np.log2(P2 / P), 0.0)
            eA = np.where(A != 0.0, np.log2(A2 / A), 0.0)
        assert np.allclose(eP, np.rint(eP), atol=1e-9) and np.allclose(eA, np.rint(eA), atol=1e-9), "an entry is not a monomial in one duration"
        nc = 2 * r
        for i in range(M):
            cols = np.zeros(n, dtype=bool)
            cols[i * nc:(i + 1) * nc] = True
            dP = np.where(cols[None, :] & cols[:, None], np.rint(eP) * P / T[i], 0.0)
            dA = np.where(cols[None, :], np.rint(eA) * A / T[i], 0.0)
            dK.append((dP, dA))
        return K, n, B, dK, P

    def grad(self, p, T):
        """-> (parts dict, df/dp [M + 1][3], df/dT [M])"""
        q = self.parts(p, T)
        r, M = self.r, self.M
        K, n, B, dK, P = self._kkt(T)
        gphi = (np.asarray(q["lim"]["grad_coeff"], dtype=np.float64) + np.asarray(q["clr"]["grad_coeff"], dtype=np.float64)).reshape(3, -1)
        gp = np.zeros((M + 1, 3))
        gT = self.wt + np.asarray(q["lim"]["grad_times"], dtype=np.float64) + np.asarray(q["clr"]["grad_times"], dtype=np.float64)
        for ax in range(3):
            b = self.o.bounds(r, p[:, ax], self.bc[0, :, ax], self.bc[1, :, ax])[0]
            zed = np.linalg.solve(K, np.concatenate([np.zeros(n), b]))
            c, lam = q["c"][ax].ravel(), zed[n:]
            g = self.ws * 2.0 * (P @ c) + gphi[ax]
            y = np.linalg.solve(K, np.concatenate([g, np.zeros(K.shape[0] - n)]))
            yc, yl = y[:n], y[n:]
            gp[:, ax] = yl @ B
            for i, (dP, dA) in enumerate(dK):
                gT[i] += self.ws * (c @ dP @ c) - (yc @ (2.0 * dP) @ c + yc @ (dA.T @ lam) + yl @ (dA @ c))
        return q, gp, gT


def iterate(prob, max_iters, **params):
    """The iteration of the header on one trajectory.  -> dict p, T (result), f_start, f, history [max_iters] (f_best after each trial),
    accepted, peak [2], min_dist, outside (at the result)"""
    P = dict(PARAMS, **params)
    M, r = prob.M, prob.r
    p, T = prob.start_p.copy(), clamp_times(prob.start_T, **params)
    lo, hi = prob.start_p - P["max_move"], prob.start_p + P["max_move"]
    inner = np.zeros((M + 1, 1), dtype=bool)
    inner[1:M] = True

    def directions(gp, gT, p, T):
        s = np.ones(M + 1)
        s[1:M] = T[:-1] ** -(2 * r - 1) + T[1:] ** -(2 * r - 1)
        dp = gp / s[:, None]
        dp[((p <= lo) & (dp > 0)) | ((p >= hi) & (dp < 0))] = 0.0
        du = T * gT
        du[((T <= P["t_min"]) & (du > 0)) | ((T >= P["t_max"]) & (du < 0))] = 0.0
        return np.where(inner, dp, 0.0), du

    q, gp, gT = prob.grad(p, T)
    f_best = f_start = q["f"]
    dp, du = directions(gp, gT, p, T)
    mp, mu = float(np.max(np.abs(dp))), float(np.max(np.abs(du)))
    sig_p = P["initial_step_move"] / mp if 0.0 < mp < np.inf else 0.0
    sig_u = P["initial_step_log"] / mu if 0.0 < mu < np.inf else 0.0
    alpha = 1.0 if (sig_p > 0.0 or sig_u > 0.0) else 0.0
    history, accepted = [], 0
    for _ in range(max_iters):
        dp, du = directions(gp, gT, p, T)
        pt = np.where(inner, np.minimum(np.maximum(p - alpha * sig_p * dp, lo), hi), p)
        Tt = np.minimum(np.maximum(T * np.exp(-alpha * sig_u * du), P["t_min"]), P["t_max"])
        need = P["armijo_c"] * (float(np.sum(gp * (p - pt))) + float(np.sum(du * np.log(T / Tt))))
        ok = False
        if alpha > 0.0:
            q_t, gp_t, gT_t = prob.grad(pt, Tt)
            ok = q_t["f"] <= f_best - need
        if ok:
            p, T, q, gp, gT, f_best = pt, Tt, q_t, gp_t, gT_t, q_t["f"]
            accepted += 1
        alpha *= P["grow"] if ok else P["shrink"]
        history.append(f_best)
    return dict(p=p, T=T, f_start=f_start, f=f_best, history=np.array(history), accepted=accepted, peak=q["peak"], min_dist=q["min_dist"],
                outside=q["outside"])


def lbfgsb(prob, **params):
    """scipy's L-BFGS-B on f from the start in x = (interior p, log T), the box and the log bounds as bounds.  -> dict p, T, f, peak, min_dist, outside"""
    from scipy.optimize import minimize
    P = dict(PARAMS, **params)
    M = prob.M
    T0 = clamp_times(prob.start_T, **params)
    n_p = 3 * (M - 1)
    # scipy sees the variables in units of the iteration's first step (initial_step_move metres, initial_step_log in log T): its own first
    # step has length one in ITS variables, which in metres and in log T would land far up the flank of a penalty
    unit = np.concatenate([np.full(n_p, P["initial_step_move"]), np.full(M, P["initial_step_log"])])
    x0 = np.concatenate([prob.start_p[1:M].ravel(), np.log(T0)]) / unit

    def unpack(x):
        x = x * unit
        p = prob.start_p.copy()
        p[1:M] = x[:n_p].reshape(M - 1, 3)
        return p, np.exp(x[n_p:])

    def fg(x, c=1.0):
        p, T = unpack(x)
        q, gp, gT = prob.grad(p, T)
        return c * q["f"], c * np.concatenate([gp[1:M].ravel(), T * gT]) * unit
    half = P["max_move"] / P["initial_step_move"]
    bounds = list(zip(x0[:n_p] - half, x0[:n_p] + half)) + [(math.log(P["t_min"]) / P["initial_step_log"], math.log(P["t_max"]) / P["initial_step_log"])] * M
    # ... and f in units of its largest gradient component at the start: L-BFGS-B's first model has unit curvature, and a gradient of 1e7
    # (a start far outside the limits) would send its first Cauchy point straight into the corners of the box
    g0 = float(np.max(np.abs(fg(x0)[1])))
    c = 1.0 / g0 if 0.0 < g0 < math.inf else 1.0
    # (restarted from its own result while that still helps: the memory of a run that crossed a kink of the penalty may stall it)
    x, f_last = x0, math.inf
    for _ in range(3):
        res = minimize(fg, x, args=(c,), jac=True, method="L-BFGS-B", bounds=bounds,
                       options=dict(maxiter=500, maxfun=1000, maxls=40, ftol=1e-14, gtol=1e-10 * c))
        x = res.x
        if not res.fun < f_last * (1.0 - 1e-9):
            break
        f_last = res.fun
    p, T = unpack(x)
    q = prob.parts(p, T)
    return dict(p=p, T=T, f=q["f"], peak=q["peak"], min_dist=q["min_dist"], outside=q["outside"])
