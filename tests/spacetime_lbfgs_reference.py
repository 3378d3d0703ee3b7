"""A designed reference of the joint waypoint / duration optimiser with limited-memory BFGS directions (include/uavqp.h:
uavqp_spacetime_lbfgs_device), numpy only, written from the header text and not from the kernel.  Built on tests/spacetime_reference.py: the
same Problem (the oracle's exact solve, the longdouble penalties, the adjoint gradient), the same cases, limits, seeds and scipy records.
Shared by tests/test_spacetime_lbfgs_contract.py (CPU), tests/test_gpu_spacetime_lbfgs.py and tools/spacetime_convergence.py --method lbfgs.

  iterate_lbfgs()   the iteration of the header on one trajectory, one trial per step, f after every trial

Variables of the method: x = (p_k[axis] / initial_step_move for the interior knots, log T_i / initial_step_log), the units
spacetime_reference.lbfgsb hands to scipy; g = (initial_step_move df/dp, initial_step_log T_i df/dT_i)."""
import numpy as np

import spacetime_reference as R

PARAMS = dict(R.PARAMS, memory=8, max_backtracks=6, curvature_eps=1e-10)
DEFAULT_MAX_ITERS = 32
STEPS = (16, 32, 64, 128)
FEASIBILITY_ITERS = 64
DESCENT_EPS = 1e-10
# The worst fraction of scipy's decrease the transcription leaves on cases(r) and uniform_cases(r), r = 3 and 4, after the default 32 trials
# with the default memory and max_backtracks (tools/spacetime_convergence.py --method lbfgs; DESIGN.md section 5.21 has the whole table), and
# the trajectory it is attained at.
GAP_LBFGS_AT_DEFAULT = 9.965e-4
GAP_LBFGS_CASE = (3, "ragged", 9)


def iterate_lbfgs(prob, max_iters, **params):
    """-> dict p, T (result), f_start, f, history [max_iters] (f_best after each trial), accepted, stored (pairs that passed the curvature
    test), resets (entries into gradient mode after the start), peak [2], min_dist, outside (at the result)"""
    P = dict(PARAMS, **params)
    M, r = prob.M, prob.r
    sm, sl = P["initial_step_move"], P["initial_step_log"]
    t_min, t_max = P["t_min"], P["t_max"]
    p, T = prob.start_p.copy(), R.clamp_times(prob.start_T, **{k: v for k, v in params.items() if k in R.PARAMS})
    lo, hi = prob.start_p - P["max_move"], prob.start_p + P["max_move"]
    inner = np.zeros((M + 1, 1), dtype=bool)
    inner[1:M] = True

    def vec(a_p, a_u):
        return np.concatenate([a_p[1:M].ravel(), a_u])

    def blocked(p, T, gp, gT):
        bp = (((p <= lo) & (gp > 0)) | ((p >= hi) & (gp < 0))) & inner
        gu = T * gT
        bu = ((T <= t_min) & (gu > 0)) | ((T >= t_max) & (gu < 0))
        return bp, bu

    def gradient_directions(p, T, gp, gT):
        """d^p = g^p / s_k, d^u = T g^T, blocked components zero (the direction of the projected-gradient entry)"""
        s = np.ones(M + 1)
        s[1:M] = T[:-1] ** -(2 * r - 1) + T[1:] ** -(2 * r - 1)
        bp, bu = blocked(p, T, gp, gT)
        dp = np.where(inner & ~bp, gp / s[:, None], 0.0)
        du = np.where(bu, 0.0, T * gT)
        return dp, du

    def enter_gradient_mode(p, T, gp, gT):
        dp, du = gradient_directions(p, T, gp, gT)
        mp, mu = float(np.max(np.abs(dp))), float(np.max(np.abs(du)))
        sig_p = sm / mp if 0.0 < mp < np.inf else 0.0
        sig_u = sl / mu if 0.0 < mu < np.inf else 0.0
        return sig_p, sig_u, (1.0 if (sig_p > 0.0 or sig_u > 0.0) else 0.0)

    def two_loop(p, T, gp, gT, pairs):
        """-> the quasi-Newton direction in x (blocked components zero), or None: clear the memory and enter gradient mode"""
        bp, bu = blocked(p, T, gp, gT)
        free = ~vec(bp, bu)
        g = np.where(free, vec(sm * gp, sl * T * gT), 0.0)
        s_new, y_new = pairs[-1]
        sy, yy = float(np.sum((s_new * y_new)[free])), float(np.sum((y_new * y_new)[free]))
        gamma = sy / yy if yy > 0.0 else 0.0
        if not (0.0 < gamma < np.inf):
            return None
        q, a = g.copy(), []
        for s, y in reversed(pairs):
            rho = float(np.sum((s * y)[free]))
            if not rho > 0.0:
                a.append(None)
                continue
            aj = float(np.sum((s * q)[free])) / rho
            q = np.where(free, q - aj * y, 0.0)
            a.append(aj)
        z = gamma * q
        for (s, y), aj in zip(pairs, reversed(a)):
            if aj is None:
                continue
            b = float(np.sum((y * z)[free])) / float(np.sum((s * y)[free]))
            z = np.where(free, z + (aj - b) * s, 0.0)
        d = -z
        gd = float(g @ d)
        if not gd < -DESCENT_EPS * float(np.sqrt(g @ g)) * float(np.sqrt(d @ d)):
            return None
        return d

    q0, gp, gT = prob.grad(p, T)
    f_best = f_start = q0["f"]
    at = q0
    sig_p, sig_u, alpha = enter_gradient_mode(p, T, gp, gT)
    pairs, d_qn, rejects = [], None, 0          # d_qn None: gradient mode
    history, accepted, stored, resets = [], 0, 0, 0
    n_p = 3 * (M - 1)
    for _ in range(max_iters):
        if d_qn is None:
            dp, du = gradient_directions(p, T, gp, gT)
            pt = np.where(inner, np.minimum(np.maximum(p - alpha * sig_p * dp, lo), hi), p)
            Tt = np.minimum(np.maximum(T * np.exp(-alpha * sig_u * du), t_min), t_max)
        else:
            step_p = np.zeros_like(p)
            step_p[1:M] = d_qn[:n_p].reshape(M - 1, 3)
            pt = np.where(inner, np.minimum(np.maximum(p + alpha * sm * step_p, lo), hi), p)
            Tt = np.minimum(np.maximum(T * np.exp(alpha * sl * d_qn[n_p:]), t_min), t_max)
        need = P["armijo_c"] * (float(np.sum((gp * (p - pt))[1:M])) + float(np.sum(T * gT * np.log(T / Tt))))
        ok = False
        if alpha > 0.0:
            q_t, gp_t, gT_t = prob.grad(pt, Tt)
            ok = q_t["f"] <= f_best - need
        if ok:
            s = vec((pt - p) / sm, np.log(Tt / T) / sl)
            y = vec(sm * (gp_t - gp), sl * (Tt * gT_t - T * gT))
            if float(s @ y) > P["curvature_eps"] * float(np.sqrt(s @ s)) * float(np.sqrt(y @ y)):
                pairs = (pairs + [(s, y)])[-int(P["memory"]):]
                stored += 1
            p, T, at, gp, gT, f_best = pt, Tt, q_t, gp_t, gT_t, q_t["f"]
            accepted += 1
            rejects = 0
            if pairs:
                d_qn = two_loop(p, T, gp, gT, pairs)
                alpha = 1.0
                if d_qn is None:
                    pairs, resets = [], resets + 1
                    sig_p, sig_u, alpha = enter_gradient_mode(p, T, gp, gT)
            else:
                alpha *= P["grow"]
        else:
            alpha *= P["shrink"]
            if d_qn is not None:
                rejects += 1
                if rejects >= int(P["max_backtracks"]):
                    pairs, d_qn, rejects, resets = [], None, 0, resets + 1
                    sig_p, sig_u, alpha = enter_gradient_mode(p, T, gp, gT)
        history.append(f_best)
    return dict(p=p, T=T, f_start=f_start, f=f_best, history=np.array(history), accepted=accepted, stored=stored, resets=resets,
                peak=at["peak"], min_dist=at["min_dist"], outside=at["outside"])
