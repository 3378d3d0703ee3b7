"""A designed reference of the swarm optimiser (include/uavqp.h: uavqp_swarm_optimize_device), numpy only, written from the header text and
not from the kernels.  It COMPOSES the two references that exist: tests/spacetime_reference.py (Problem: f_b and its gradient per vehicle
on the oracle's exact solve) and tests/swarm_reference.py (swarm: Phi_swarm, its gradient in the coefficients -- fed into each vehicle's
adjoint solve here -- and its explicit gradients in the durations and the departures).  Shared by tests/test_swarm_opt_contract.py (CPU),
tests/test_gpu_swarm_opt.py, tests/test_gpu_swarm_opt_facade.py and tools/swarm_opt_convergence.py.

  SwarmProblem      one swarm: f_g(p, T, start) = sum_b [ smooth_weight J_b + time_weight sum T_b + Phi_flight,b ] + Phi_swarm,g over the
                    vehicles that take part, and its total gradient in every waypoint, duration and departure
  iterate_swarm()   the projected-gradient / Armijo iteration of the header, ONE accept / reject per swarm and trial
  lbfgsb_swarm()    scipy's L-BFGS-B on all variables of one swarm from the same start (tools only: the tests read recorded optima)
  batch_of()        the batches the tests fly: swarm_reference.scene flights inside the map of waypoint_opt_reference.scene

Flights.  CENTRE / RADIUS put the circle of swarm_reference.scene into the free quadrant of the map next to the pillar (x, y in -3.5 .. -0.3
against the pillar's -0.25 .. 0.5): the chords that pass nearest the pillar come inside the clearance band (d_safe 0.5 m), so the
clearance part is active in some vehicles and no sample leaves the map.  FLIGHT seconds over chords of about 3.2 m: the jitter of
swarm_reference.scene on the knots of an eleven-segment vehicle asks for accelerations of several m/s^2 at any shorter flight, and the
limit penalty would then be 1e7 and more against a swarm penalty of 1e3.  LIMITS (one set for r = 3 and 4) is exceeded by the vehicles
of many segments at the start and by most once time_weight has shortened the flights.  SWARM: the clock covers the staggered departures
and the whole flight (-0.4 .. 7.6 s); d_safe 0.8 m makes most vehicles of a swarm meet at the centre.
SEEDS: tools/swarm_opt_convergence.py --seed-search, the first seed from 1 per r for which, on the ragged batch (seed) and the uniform
batch (100 + seed), from the reference alone: no sample outside the map at the start and at the transcription's results; every swarm of
two or more has Phi_swarm > 0 at the start; and in at least half of those swarms the transcription's run with swarm weight = 0 ends with a
smallest separation below d_safe and the penalised run ends with a larger one."""
import math

import numpy as np

import spacetime_reference as R
import swarm_reference as S

CENTRE, RADIUS, FLIGHT = (-1.9, -1.9, 1.3), 1.6, 6.0
SWARM = dict(n_samples=80, clock_start=-0.4, dt=0.1, d_safe=0.8, downwash=1.0, weight=1e3)
LIMITS = dict(samples_per_seg=8, v_max=1.2, a_max=2.5, weight_v=1e3, weight_a=1e3)
PARAMS = dict(R.PARAMS, start_window=0.0, initial_step_start=0.1)
# swarms of the ragged batch (segments per vehicle: swarms of 1, 2, 3 and 5 vehicles, M in 1 .. 11, M = 1 among them) and of the uniform one
RAGGED = ((4,), (3, 1), (2, 5, 3), (6, 1, 11, 2, 4))
UNIFORM_M = 8
UNIFORM = ((UNIFORM_M,) * 2, (UNIFORM_M,) * 3)
SEEDS = {3: 1, 4: 1}
STEPS = (16, 32, 64, 128)
# The worst fraction of scipy's decrease the transcription leaves on the swarms of batch_of(r, "ragged") and batch_of(r, "uniform"), r = 3
# and 4, after the library's default max_iters (tools/swarm_opt_convergence.py; DESIGN.md section 5.23 has the whole table), and the
# swarm it is attained at.
DEFAULT_MAX_ITERS = 32
GAP_AT_DEFAULT = 8.981e-2
GAP_CASE = (3, "uniform", 0)


def batch(r, groups, seed, centre=CENTRE):
    """A batch of swarms in the C-ABI layout.  groups: per swarm the segments per vehicle.  -> dict r, seg_offsets, waypoints, times, bc,
    group_offsets, start"""
    rng = np.random.default_rng(seed)
    wps, Ts, starts, Ms = [], [], [], []
    for Mg in groups:
        w, T, s = S.scene(rng, list(Mg), centre=centre, radius=RADIUS, flight=FLIGHT)
        wps += w
        Ts += T
        starts += list(s)
        Ms += list(Mg)
    n = len(Ms)
    bc = np.zeros((n, 2, r - 1, 3))
    bc[::2, :, 0, :] = rng.uniform(-0.3, 0.3, size=bc[::2, :, 0, :].shape)   # every other vehicle starts and ends moving
    so = np.zeros(n + 1, dtype=np.int32)
    so[1:] = np.cumsum(Ms)
    go = np.zeros(len(groups) + 1, dtype=np.int32)
    go[1:] = np.cumsum([len(Mg) for Mg in groups])
    return dict(r=r, seg_offsets=so, waypoints=np.vstack(wps), times=np.concatenate(Ts), bc=bc, group_offsets=go,
                start=np.array(starts, dtype=np.float64))


def batch_of(r, kind, seed=None):
    seed = SEEDS[r] if seed is None else seed
    if kind == "ragged":
        return batch(r, RAGGED, 1000 * r + seed)
    return batch(r, UNIFORM, 1000 * r + 100 + seed)


def vehicles(b, g):
    """the trajectories of swarm g of a batch"""
    return list(range(int(b["group_offsets"][g]), int(b["group_offsets"][g + 1])))


class SwarmProblem:
    """f_g(p, T, start) of one swarm.  ps: list of [M_b + 1][3], Ts: list of [M_b], starts [A].  live[b] False: the vehicle takes no part
    (it is left out of f_g and of every pair)."""

    def __init__(self, oracle, r, wps, Ts, bcs, starts, live=None, limits=None, clearance=None, swarm=None, smooth_weight=PARAMS["smooth_weight"],
                 time_weight=PARAMS["time_weight"], sc=None):
        self.r, self.A = r, len(Ts)
        self.veh = [R.Problem(oracle, r, wp, T, bc, limits=dict(LIMITS, **(limits or {})), clearance=clearance, smooth_weight=smooth_weight, time_weight=time_weight,
                              sc=sc) for wp, T, bc in zip(wps, Ts, bcs)]
        self.start_s = np.array(starts, dtype=np.float64)
        self.live = [True] * self.A if live is None else [bool(x) for x in live]
        self.sp = dict(SWARM, **(swarm or {}))

    @classmethod
    def of_batch(cls, oracle, b, g, **kw):
        bs = vehicles(b, g)
        parts = [R.split(b, t) for t in bs]
        return cls(oracle, b["r"], [q[0] for q in parts], [q[1] for q in parts], [q[2] for q in parts], b["start"][bs], **kw)

    def start(self):
        return [v.start_p.copy() for v in self.veh], [v.start_T.copy() for v in self.veh], self.start_s.copy()

    def parts(self, ps, Ts, starts, grads=False):
        """-> dict f, phi_swarm, veh (the per-vehicle dicts of Problem.parts, None for a vehicle that takes no part), swarm (swarm_reference's)"""
        qs = [v.parts(p, T) if l else None for v, p, T, l in zip(self.veh, ps, Ts, self.live)]
        Cs = [q["c"] if q is not None else np.zeros((3, len(T), 2 * self.r)) for q, T in zip(qs, Ts)]
        sw = S.swarm(self.r, [np.asarray(T) for T in Ts], Cs, list(starts), self.live, grads=grads, **self.sp)
        f = float(sum(q["f"] for q in qs if q is not None) + float(sw["phi"]))
        return dict(f=f, phi_swarm=float(sw["phi"]), veh=qs, swarm=sw, min_sep=np.asarray(sw["min_sep"], dtype=np.float64))

    def f(self, ps, Ts, starts):
        return self.parts(ps, Ts, starts)["f"]

    def grad(self, ps, Ts, starts):
        """-> (parts dict, df/dp list of [M + 1][3], df/dT list of [M], df/dstart [A]); zeros for a vehicle that takes no part"""
        q = self.parts(ps, Ts, starts, grads=True)
        sw = q["swarm"]
        gps, gTs = [], []
        for b, v in enumerate(self.veh):
            if not self.live[b]:
                gps.append(np.zeros_like(ps[b]))
                gTs.append(np.zeros(len(Ts[b])))
                continue
            gp, gT = _vehicle_grad(v, q["veh"][b], ps[b], Ts[b], np.asarray(sw["grad_coeff"][b], dtype=np.float64),
                                   np.asarray(sw["grad_times"][b], dtype=np.float64))
            gps.append(gp)
            gTs.append(gT)
        gs = np.where(self.live, np.asarray(sw["grad_start"], dtype=np.float64), 0.0)
        return q, gps, gTs, gs


def _vehicle_grad(v, q, p, T, g_extra, gt_extra):
    """Problem.grad of tests/spacetime_reference.py with one more penalty: g_extra [3][M][2r] joins dPhi/dc BEFORE the adjoint solve (one
    solve takes the sum through the minimiser), gt_extra [M] joins the explicit time gradients."""
    r, M = v.r, v.M
    K, n, B, dK, P = v._kkt(T)
    gphi = (np.asarray(q["lim"]["grad_coeff"], dtype=np.float64) + np.asarray(q["clr"]["grad_coeff"], dtype=np.float64)).reshape(3, -1)
    gphi = gphi + g_extra.reshape(3, -1)
    gp = np.zeros((M + 1, 3))
    gT = v.wt + np.asarray(q["lim"]["grad_times"], dtype=np.float64) + np.asarray(q["clr"]["grad_times"], dtype=np.float64) + gt_extra
    for ax in range(3):
        b = v.o.bounds(r, p[:, ax], v.bc[0, :, ax], v.bc[1, :, ax])[0]
        zed = np.linalg.solve(K, np.concatenate([np.zeros(n), b]))
        c, lam = q["c"][ax].ravel(), zed[n:]
        g = v.ws * 2.0 * (P @ c) + gphi[ax]
        y = np.linalg.solve(K, np.concatenate([g, np.zeros(K.shape[0] - n)]))
        yc, yl = y[:n], y[n:]
        gp[:, ax] = yl @ B
        for i, (dP, dA) in enumerate(dK):
            gT[i] += v.ws * (c @ dP @ c) - (yc @ (2.0 * dP) @ c + yc @ (dA.T @ lam) + yl @ (dA @ c))
    return gp, gT


def _directions(prob, P, gps, gTs, gs, ps, Ts, s, lo_p, hi_p, lo_s, hi_s):
    """d^p, d^u per vehicle and d^s, each zero where its bound blocks it (the header's rules)"""
    r = prob.r
    dps, dus = [], []
    for b in range(prob.A):
        M = len(Ts[b])
        inner = np.zeros((M + 1, 1), dtype=bool)
        inner[1:M] = True
        sc = np.ones(M + 1)
        sc[1:M] = Ts[b][:-1] ** -(2 * r - 1) + Ts[b][1:] ** -(2 * r - 1)
        dp = gps[b] / sc[:, None]
        dp[((ps[b] <= lo_p[b]) & (dp > 0)) | ((ps[b] >= hi_p[b]) & (dp < 0))] = 0.0
        du = Ts[b] * gTs[b]
        du[((Ts[b] <= P["t_min"]) & (du > 0)) | ((Ts[b] >= P["t_max"]) & (du < 0))] = 0.0
        live = prob.live[b]
        dps.append(np.where(inner & live, dp, 0.0))
        dus.append(du if live else np.zeros(M))
    ds = gs.copy()
    ds[((s <= lo_s) & (ds > 0)) | ((s >= hi_s) & (ds < 0))] = 0.0
    return dps, dus, np.where(prob.live, ds, 0.0)


def iterate_swarm(prob, max_iters, **params):
    """The iteration of the header on one swarm.  -> dict p, T (lists), start, f_start, f, history [max_iters] (f_g after each trial),
    accepted, min_sep [A], parts (Problem.parts per vehicle at the result)"""
    P = dict(PARAMS, **params)
    ps, Ts, s = prob.start()
    Ts = [R.clamp_times(T, **{k: P[k] for k in ("t_min", "t_max")}) for T in Ts]
    lo_p, hi_p = [p - P["max_move"] for p in ps], [p + P["max_move"] for p in ps]
    lo_s, hi_s = s - P["start_window"], s + P["start_window"]
    q, gps, gTs, gs = prob.grad(ps, Ts, s)
    f_best = f_start = q["f"]

    def vmax(xs):
        return max([float(np.max(np.abs(x))) for x, l in zip(xs, prob.live) if l and np.size(x)] + [0.0])
    dps, dus, ds = _directions(prob, P, gps, gTs, gs, ps, Ts, s, lo_p, hi_p, lo_s, hi_s)
    mp, mu, ms = vmax(dps), vmax(dus), float(np.max(np.abs(ds))) if ds.size else 0.0
    sig_p = P["initial_step_move"] / mp if 0.0 < mp < np.inf else 0.0
    sig_u = P["initial_step_log"] / mu if 0.0 < mu < np.inf else 0.0
    sig_s = P["initial_step_start"] / ms if 0.0 < ms < np.inf else 0.0
    alpha = 1.0 if (sig_p > 0.0 or sig_u > 0.0 or sig_s > 0.0) else 0.0
    if not (any(prob.live) and math.isfinite(f_start)):
        alpha = 0.0
    history, accepted = [], 0
    for _ in range(max_iters):
        dps, dus, ds = _directions(prob, P, gps, gTs, gs, ps, Ts, s, lo_p, hi_p, lo_s, hi_s)
        pts = [np.minimum(np.maximum(p - alpha * sig_p * dp, lo), hi) for p, dp, lo, hi in zip(ps, dps, lo_p, hi_p)]
        pts = [np.where(dp != 0.0, pt, p) for p, pt, dp in zip(ps, pts, dps)]
        Tts = [np.minimum(np.maximum(T * np.exp(-alpha * sig_u * du), P["t_min"]), P["t_max"]) for T, du in zip(Ts, dus)]
        st = np.minimum(np.maximum(s - alpha * sig_s * ds, lo_s), hi_s)
        need = sum(float(np.sum(gp * (p - pt))) + float(np.sum(du * np.log(T / Tt))) for gp, p, pt, du, T, Tt in zip(gps, ps, pts, dus, Ts, Tts))
        need = P["armijo_c"] * (need + float(np.sum(ds * (s - st))))
        ok = False
        if alpha > 0.0:
            q_t, gps_t, gTs_t, gs_t = prob.grad(pts, Tts, st)
            ok = q_t["f"] <= f_best - need
        if ok:
            ps, Ts, s, q, gps, gTs, gs, f_best = pts, Tts, st, q_t, gps_t, gTs_t, gs_t, q_t["f"]
            accepted += 1
        alpha *= P["grow"] if ok else P["shrink"]
        history.append(f_best)
    return dict(p=ps, T=Ts, start=s, f_start=f_start, f=f_best, history=np.array(history), accepted=accepted, min_sep=q["min_sep"],
                parts=q["veh"], phi_swarm=q["phi_swarm"])


def lbfgsb_swarm(prob, **params):
    """scipy's L-BFGS-B on f_g from the start in x = (interior p, log T of every vehicle, the departures if start_window > 0), in the
    units of the iteration's first step, the boxes as bounds.  -> dict p, T, start, f, min_sep"""
    from scipy.optimize import minimize
    P = dict(PARAMS, **params)
    ps0, Ts0, s0 = prob.start()
    Ts0 = [R.clamp_times(T, **{k: P[k] for k in ("t_min", "t_max")}) for T in Ts0]
    with_s = P["start_window"] > 0.0
    Ms = [len(T) for T in Ts0]
    n_p = [3 * (M - 1) for M in Ms]
    unit = np.concatenate([np.concatenate([np.full(n, P["initial_step_move"]), np.full(M, P["initial_step_log"])]) for n, M in zip(n_p, Ms)]
                          + ([np.full(prob.A, P["initial_step_start"])] if with_s else []))
    x0 = np.concatenate([np.concatenate([p[1:M].ravel(), np.log(T)]) for p, T, M in zip(ps0, Ts0, Ms)] + ([s0] if with_s else [])) / unit

    def unpack(x):
        x = x * unit
        ps, Ts, at = [], [], 0
        for b, M in enumerate(Ms):
            p = ps0[b].copy()
            p[1:M] = x[at:at + n_p[b]].reshape(M - 1, 3)
            at += n_p[b]
            ps.append(p)
            Ts.append(np.exp(x[at:at + M]))
            at += M
        return ps, Ts, (x[at:] if with_s else s0)

    def fg(x, c=1.0):
        ps, Ts, s = unpack(x)
        q, gps, gTs, gs = prob.grad(ps, Ts, s)
        g = np.concatenate([np.concatenate([gp[1:M].ravel(), T * gT]) for gp, gT, T, M in zip(gps, gTs, Ts, Ms)] + ([gs] if with_s else []))
        return c * q["f"], c * g * unit
    half = P["max_move"] / P["initial_step_move"]
    tb = (math.log(P["t_min"]) / P["initial_step_log"], math.log(P["t_max"]) / P["initial_step_log"])
    bounds, at = [], 0
    for b, M in enumerate(Ms):
        bounds += list(zip(x0[at:at + n_p[b]] - half, x0[at:at + n_p[b]] + half)) + [tb] * M
        at += n_p[b] + M
    if with_s:
        w = P["start_window"] / P["initial_step_start"]
        bounds += list(zip(x0[at:] - w, x0[at:] + w))
    g0 = float(np.max(np.abs(fg(x0)[1])))
    c = 1.0 / g0 if 0.0 < g0 < math.inf else 1.0
    x, f_last = x0, math.inf
    for _ in range(2):   # (restarted from its own result once, as spacetime_reference.lbfgsb does while that still helps)
        res = minimize(fg, x, args=(c,), jac=True, method="L-BFGS-B", bounds=bounds,
                       options=dict(maxiter=300, maxfun=600, maxls=40, ftol=1e-14, gtol=1e-10 * c))
        x = res.x
        if not res.fun < f_last * (1.0 - 1e-9):
            break
        f_last = res.fun
    ps, Ts, s = unpack(x)
    q = prob.parts(ps, Ts, s)
    return dict(p=ps, T=Ts, start=np.asarray(s, dtype=np.float64), f=q["f"], min_sep=q["min_sep"])


def evaluate(oracle, b, g, waypoints, times, start, status=None, sc=None, **kw):
    """f_g of swarm g of batch b at a point given in the C-ABI layout (what a device run hands back).  -> the dict of SwarmProblem.parts"""
    bs = vehicles(b, g)
    at = dict(b, waypoints=np.asarray(waypoints, dtype=np.float64).reshape(-1, 3), times=np.asarray(times, dtype=np.float64))
    parts = [R.split(at, t) for t in bs]
    live = None if status is None else [int(status[t]) == 1 for t in bs]
    prob = SwarmProblem(oracle, b["r"], [q[0] for q in parts], [q[1] for q in parts], [q[2] for q in parts], np.asarray(start)[bs], live=live,
                        sc=sc, **kw)
    return prob.parts(*prob.start())
