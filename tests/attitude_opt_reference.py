"""A designed reference of the joint optimiser with the attitude penalty in its objective (include/uavqp.h: uavqp_attitude_optimize_device),
numpy only.  tests/spacetime_lbfgs_reference.py extended by one term: the Problem of tests/spacetime_reference.py (the oracle's exact
solve, the longdouble penalties, the adjoint gradient) with Phi_att of tests/attitude_penalty_reference.py added to f and its two partial
gradients added to the penalties' before the adjoint solve; the iteration is iterate_lbfgs of tests/spacetime_lbfgs_reference.py unchanged,
as the device's step kernel is.  Shared by tests/golden/gen_attitude_scipy.py (CPU) and tests/test_gpu_attitude_opt.py.

Scenes.  The batches of tests/spacetime_reference.py (ragged: 14 trajectories; uniform: 8 x 4 segments) started from TIME_SCALE x their
durations: shorter flights than those of the other tests, whose optima (tilt up to 0.18 rad, body rate up to 0.65 rad/s) already lie outside
ATTITUDE.  Tilt and body rate start far outside it -- up to 0.9 rad and 30 rad/s -- and the cube of u_rate makes f_start between 7.6 and
1e10 times f_scipy (recorded per trajectory in tests/golden/attitude_scipy.json); at scipy's optimum the attitude penalty is still at
work on the ragged batch (Phi_att 0.02 .. 11 there)."""
import numpy as np

import attitude_penalty_reference as A
import spacetime_lbfgs_reference as Q
import spacetime_reference as R

TIME_SCALE = 0.8
ATTITUDE = dict(samples_per_seg=8, gravity=9.81, f_min=9.5, f_max=10.2, tilt_max=0.1, rate_max=0.3, weight_thrust=1e3, weight_tilt=1e3,
                weight_rate=1e3)
KINDS = [(3, "ragged"), (4, "uniform")]
DEFAULT_MAX_ITERS = Q.DEFAULT_MAX_ITERS
# The worst fraction of scipy's decrease the transcription (iterate_lbfgs on AttitudeProblem) leaves on the batches of KINDS after the
# default 32 trials, and where (tests/golden/gen_attitude_scipy.py prints it; the per-trajectory figures are in the golden file).
GAP_ATTITUDE_AT_DEFAULT = 7.680e-6
GAP_ATTITUDE_CASE = (3, "ragged", 9)


def batch_of(r, kind):
    b = R.batch_of(r, kind)
    return dict(b, times=b["times"] * TIME_SCALE)


class AttitudeProblem(R.Problem):
    """f of R.Problem + Phi_att; grad() is R.Problem.grad, fed with the summed partial gradients of all three penalties."""

    def __init__(self, oracle, r, wp, T, bc, attitude=None, **kw):
        super().__init__(oracle, r, wp, T, bc, **kw)
        self.ap = dict(ATTITUDE, **(attitude or {}))

    def parts(self, p, T):
        q = super().parts(p, T)
        att = A.penalty(self.r, [0, self.M], T, q["c"].ravel(), **self.ap)
        phi_att = float(att["phi"][0])
        lim = dict(q["lim"])     # (grad() adds lim and clr: the attitude term rides on lim's two gradients)
        lim["grad_coeff"] = np.asarray(lim["grad_coeff"], dtype=np.float64) + np.asarray(att["grad_coeff"], dtype=np.float64)
        lim["grad_times"] = np.asarray(lim["grad_times"], dtype=np.float64) + np.asarray(att["grad_times"], dtype=np.float64)
        return dict(q, f=q["f"] + phi_att, phi=q["phi"] + phi_att, lim=lim, att=att, phi_att=phi_att,
                    attitude_peak=np.asarray(att["peak"][0], dtype=np.float64))


def problem_of(oracle, r, kind, t, **kw):
    wp, T, bc = R.split(batch_of(r, kind), t)
    return AttitudeProblem(oracle, r, wp, T, bc, **kw)


def iterate(prob, max_iters=DEFAULT_MAX_ITERS, **params):
    return Q.iterate_lbfgs(prob, max_iters, **params)
