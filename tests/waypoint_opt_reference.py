"""A designed reference of the waypoint optimiser (include/uavqp.h: uavqp_cost_waypoint_gradient_device, uavqp_waypoint_optimize_device),
numpy only, written from the header text and not from the kernels: the objective on the oracle's exact solve and tests/esdf_reference.py's
longdouble penalty, the closed-form gradient, and a transcription of the iteration.  Shared by tests/test_waypoint_opt_contract.py (CPU),
tests/test_gpu_waypoint_opt.py and tools/waypoint_opt_convergence.py; the scene and the cases of those tests are built here, once.

  scene()      32 x 32 x 16 voxels of 0.25 m from (-4, -4, 0): a pillar of 3 x 3 voxels over the full height whose axis is (0.125, 0.125),
               and a slab two voxels thick at z = 3.0 .. 3.5 over |x|, |y| < 2
  cases(r)     paths of 2 .. 6 segments (plus one of 11 and one of 1) that cross the pillar with a lateral offset of 0.1 .. 0.35 m from its axis
  Problem      one trajectory: f, J, Phi, df/dp (closed form + the penalty's coefficient gradient through the LINEAR map p -> c*(p))
  iterate()    the projected-gradient / Armijo iteration of the header, one trial per step, f after every trial
  lbfgsb()     scipy's L-BFGS-B on the same f, the same start, the box as bounds
"""
import math

import numpy as np

import esdf_reference as E

LD = np.longdouble
ORIGIN, RES, DIMS, MAX_DIST = (-4.0, -4.0, 0.0), 0.25, (32, 32, 16), 10000.0
PILLAR_AXIS = np.array([0.125, 0.125])
CLEARANCE = dict(samples_per_seg=8, d_safe=0.5, weight=1e3)
PARAMS = dict(smooth_weight=1.0, max_move=1.0, initial_step=0.1, armijo_c=1e-4, shrink=0.5, grow=2.0)

_scene = None


def scene():
    """-> dict occ uint8 [32][32][16], dist float64 (the longdouble brute-force field rounded once), origin, res, max_dist"""
    global _scene
    if _scene is None:
        occ = np.zeros(DIMS, dtype=np.uint8)
        occ[15:18, 15:18, :] = 1          # pillar: x, y in -0.25 .. 0.5
        occ[8:24, 8:24, 12:14] = 1        # slab: z in 3.0 .. 3.5
        f = E.field(occ, RES, MAX_DIST)
        _scene = dict(occ=occ, dist=f["dist"].astype(np.float64), origin=ORIGIN, res=RES, max_dist=MAX_DIST)
    return _scene


def one_path(rng, M, ragged):
    """A path of M segments across the pillar: straight through a point at 0.1 .. 0.35 m beside the pillar's axis, knots jittered."""
    ang = rng.uniform(0.0, 2.0 * math.pi)
    u = np.array([math.cos(ang), math.sin(ang)])
    nrm = np.array([-u[1], u[0]])
    off = rng.uniform(0.1, 0.35) * rng.choice([-1.0, 1.0])
    half = rng.uniform(2.0, 2.6)
    s = np.linspace(-half, half, M + 1)
    if M > 1:
        s[1:-1] += rng.uniform(-0.15, 0.15, size=M - 1) * (2.0 * half / M)
    xy = PILLAR_AXIS[None, :] + off * nrm[None, :] + s[:, None] * u[None, :]
    xy[1:-1] += rng.uniform(-0.08, 0.08, size=(M - 1, 2)) if M > 1 else 0.0
    z = rng.uniform(1.0, 2.3) + rng.uniform(-0.1, 0.1, size=M + 1)
    wp = np.column_stack([xy, z])
    seg = np.linalg.norm(np.diff(wp, axis=0), axis=1)
    T = seg / 1.0 * (rng.uniform(0.7, 1.5, size=M) if ragged else 1.0)   # about 1 m/s
    return wp, T


def cases(r, seed=None, Ms=None, ragged_times=True, with_bc=True):
    """-> dict r, seg_offsets int32, waypoints [sum (M + 1)][3], times [sum M], bc [n][2][r-1][3].  Default: the ragged batch of the tests,
    14 trajectories: M = 2 .. 6 twice over, 11, 1, 3, 5.  Seeds: SEEDS[r], chosen on the CPU (tools/waypoint_opt_convergence.py) as the first
    seed from 1 for which every trajectory with an interior knot has f_start > 1.5 f_scipy, outside == 0 at the start, at scipy's optimum and
    at the transcription's result, and a larger smallest distance at that result than at the start."""
    seed = SEEDS[r] if seed is None else seed
    Ms = [2, 3, 4, 5, 6, 2, 3, 4, 5, 6, 11, 1, 3, 5] if Ms is None else Ms
    rng = np.random.default_rng(seed)
    wps, Ts = [], []
    for M in Ms:
        wp, T = one_path(rng, M, ragged_times)
        wps.append(wp)
        Ts.append(T)
    n = len(Ms)
    bc = np.zeros((n, 2, r - 1, 3))
    if with_bc:
        bc[::2, :, 0, :] = rng.uniform(-0.3, 0.3, size=bc[::2, :, 0, :].shape)   # every other trajectory starts and ends moving
    so = np.zeros(n + 1, dtype=np.int32)
    so[1:] = np.cumsum(Ms)
    return dict(r=r, seg_offsets=so, waypoints=np.vstack(wps), times=np.concatenate(Ts), bc=bc)


SEEDS = {3: 1, 4: 1}
UNIFORM_M, UNIFORM_N = 4, 8


def uniform_cases(r):
    """The uniform batch of the tests: eight trajectories of four segments, segment durations proportional to the knot spacing."""
    return cases(r, seed=100 + SEEDS[r], Ms=[UNIFORM_M] * UNIFORM_N, ragged_times=False)


def uniform11_cases(r):
    """Four trajectories of eleven segments: a segment count for which the solve has no specialised kernel, so that a uniform call and a
    ragged call of this batch run the SAME solve kernel and can be compared byte for byte (with a specialised count the two solves differ
    in their last bits, and so do the iterates).  Not compared against scipy."""
    return cases(r, seed=200 + SEEDS[r], Ms=[11] * 4, ragged_times=True)


# The worst fraction of scipy's decrease the transcription leaves on cases(r) and uniform_cases(r), r = 3 and 4, after the library's default
# of 64 trials (tools/waypoint_opt_convergence.py; after 8 / 16 / 32 / 64 / 128 trials: 0.157 / 0.111 / 0.0713 / 0.0418 / 0.0241, the
# eleven-segment trajectory of cases(3) every time).  tests/test_gpu_waypoint_opt.py allows the device twice this.
GAP_AT_DEFAULT = 4.18e-2


def split(batch, t):
    """-> (wp [M + 1][3], T [M], bc [2][r-1][3]) of trajectory t"""
    so = batch["seg_offsets"]
    s0, s1 = int(so[t]), int(so[t + 1])
    return batch["waypoints"][s0 + t:s1 + t + 1].copy(), batch["times"][s0:s1].copy(), batch["bc"][t].copy()


class Problem:
    """f(p) = smooth_weight * J(p) + Phi(c*(p), T) of one trajectory on the oracle's solve; p [M + 1][3] (the end rows are never moved)."""

    def __init__(self, oracle, r, wp, T, bc, clearance=None, smooth_weight=1.0, sc=None):
        self.o, self.r, self.T, self.bc = oracle, r, np.asarray(T, dtype=np.float64), np.asarray(bc, dtype=np.float64)
        self.M = self.T.size
        self.start = np.array(wp, dtype=np.float64)
        self.cp = dict(CLEARANCE, **(clearance or {}))
        self.ws = float(smooth_weight)
        self.sc = scene() if sc is None else sc
        self.F = (2.0 if r % 2 else -2.0) * math.factorial(2 * r - 1)
        self._S = None
        self.evals = 0

    def coeff(self, p):
        """[3][M][2r]: the oracle's exact minimiser per axis"""
        return np.array([self.o.solve_exact(self.r, p[:, ax], self.bc[0, :, ax], self.bc[1, :, ax], self.T) for ax in range(3)]).reshape(3, self.M, 2 * self.r)

    def cost(self, c):
        return sum(2.0 * self.o.cost(self.r, self.T, c[ax].ravel()) for ax in range(3))

    def penalty(self, c):
        s = self.sc
        return E.penalty(self.r, [0, self.M], self.T, c.ravel(), s["dist"], s["origin"], s["res"], s["max_dist"], **self.cp)

    def parts(self, p):
        """-> (f, J, penalty dict) at p"""
        self.evals += 1
        c = self.coeff(p)
        J, pen = self.cost(c), self.penalty(c)
        return self.ws * J + float(pen["phi"][0]), J, pen, c

    def f(self, p):
        return self.parts(p)[0]

    def S(self):
        """[2r M][M + 1]: dc*/dp of one axis.  The minimiser is linear in the positions, so column k is the solve of the unit waypoint
        e_k with zero boundary derivatives."""
        if self._S is None:
            z = np.zeros(self.r - 1)
            self._S = np.column_stack([self.o.solve_exact(self.r, np.eye(self.M + 1)[k], z, z, self.T) for k in range(self.M + 1)])
        return self._S

    def grad_J(self, c):
        """[M + 1][3]: the closed form of the header, dJ/dp_k = 2 (-1)^(r-1) (2r-1)! (c_{k-1,2r-1} - c_{k,2r-1})"""
        lead = c[:, :, -1]                                     # [3][M]
        g = np.zeros((self.M + 1, 3))
        g[1:] += self.F * lead.T
        g[:-1] -= self.F * lead.T
        return g

    def grad(self, p):
        """-> (f, df/dp [M + 1][3], J, penalty dict): closed form + the penalty's coefficient gradient through S"""
        f, J, pen, c = self.parts(p)
        gc = np.asarray(pen["grad_coeff"], dtype=np.float64).reshape(3, -1)     # [3][2r M]
        through = (gc @ self.S()).T                                              # [M + 1][3]
        return f, self.ws * self.grad_J(c) + through, J, pen


def iterate(prob, max_iters, **params):
    """The iteration of the header on one trajectory.  -> dict p (result), f_start, f (result), history [max_iters] (f_best after each
    trial), accepted, min_dist, outside (at the result)"""
    P = dict(PARAMS, **params)
    p = prob.start.copy()
    M = prob.M
    lo, hi = prob.start - P["max_move"], prob.start + P["max_move"]
    inner = np.zeros((M + 1, 1), dtype=bool)
    inner[1:M] = True
    with np.errstate(divide="ignore"):
        s = np.ones(M + 1)
        s[1:M] = prob.T[:-1] ** -(2 * prob.r - 1) + prob.T[1:] ** -(2 * prob.r - 1)

    def direction(g, p):
        d = g / s[:, None]
        d[((p <= lo) & (d > 0)) | ((p >= hi) & (d < 0))] = 0.0
        return np.where(inner, d, 0.0)

    f_best, g, _, pen = prob.grad(p)
    f_start = f_best
    dmax = np.max(np.abs(direction(g, p))) if M > 1 else 0.0
    alpha = P["initial_step"] / dmax if 0.0 < dmax < np.inf else 0.0
    history, accepted = [], 0
    for _ in range(max_iters):
        d = direction(g, p)
        trial = np.where(inner, np.minimum(np.maximum(p - alpha * d, lo), hi), p)
        need = P["armijo_c"] * float(np.sum(g * (p - trial)))
        if alpha > 0.0:
            f_t, g_t, _, pen_t = prob.grad(trial)
            ok = f_t <= f_best - need
        else:
            ok = False
        if ok:
            p, f_best, g, pen = trial, f_t, g_t, pen_t
            accepted += 1
        alpha *= P["grow"] if ok else P["shrink"]
        history.append(f_best)
    return dict(p=p, f_start=f_start, f=f_best, history=np.array(history), accepted=accepted, min_dist=float(pen["min_dist"][0]),
                outside=int(pen["outside"][0]))


def lbfgsb(prob, max_move=PARAMS["max_move"]):
    """scipy's L-BFGS-B on f from prob.start with the box as bounds (the end knots pinned by equal bounds are left out of the variables).
    -> dict p, f, outside, min_dist"""
    from scipy.optimize import minimize
    M = prob.M
    if M < 2:
        f, _, pen, _ = prob.parts(prob.start)
        return dict(p=prob.start.copy(), f=f, outside=int(pen["outside"][0]), min_dist=float(pen["min_dist"][0]))
    x0 = prob.start[1:M].ravel()

    def full(x):
        p = prob.start.copy()
        p[1:M] = x.reshape(M - 1, 3)
        return p

    def fg(x):
        f, g, _, _ = prob.grad(full(x))
        return f, g[1:M].ravel()
    res = minimize(fg, x0, jac=True, method="L-BFGS-B", bounds=list(zip(x0 - max_move, x0 + max_move)),
                   options=dict(maxiter=500, maxfun=2000, ftol=1e-13, gtol=1e-9))
    p = full(res.x)
    f, _, pen, _ = prob.parts(p)
    return dict(p=p, f=f, outside=int(pen["outside"][0]), min_dist=float(pen["min_dist"][0]))
