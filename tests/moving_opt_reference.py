"""A designed reference of the joint optimiser with the moving-obstacle penalty in its objective (include/uavqp.h:
uavqp_moving_optimize_device), numpy only.  AttitudeProblem of tests/attitude_opt_reference.py extended by the one term: Phi_moving of
tests/moving_penalty_reference.py added to f and its two partial gradients added to the penalties' before the adjoint solve; the
iteration is iterate_lbfgs of tests/spacetime_lbfgs_reference.py unchanged, as the device's step kernel is.  Shared by
tests/golden/gen_moving_scipy.py (CPU) and tests/test_gpu_moving_opt.py.

Scenes.  The batches of tests/attitude_opt_reference.py.  Every trajectory has a set of its own of two one-segment tracks at constant
velocity (about 1 m/s, mostly horizontal): the first passes within 0.2 m of the trajectory's middle waypoint at the instant the START
trajectory is there, the second within 0.2 m of the waypoint before it, each under way for 0.4 of the start flight -- both well inside
D_o = d_safe + radius >= 1 m of the start trajectory, so the term is at work from the first gradient on; on the longer trajectories the
tracks wait first and have arrived at the end.  Departures of the trajectories are spread over [0, 0.5] s and stay fixed."""
import numpy as np

import attitude_opt_reference as AO
import moving_penalty_reference as MP
import spacetime_reference as R

MOVING = dict(samples_per_seg=8, d_safe=1.0, downwash=1.0, weight=1e3)
ATTITUDE = AO.ATTITUDE
KINDS = AO.KINDS
DEFAULT_MAX_ITERS = AO.DEFAULT_MAX_ITERS
OBSTACLE_SEED = {3: 511, 4: 512}
# The worst fraction of scipy's decrease the transcription (iterate_lbfgs on MovingProblem) leaves on the batches of KINDS after the
# default 32 trials, and where (tests/golden/gen_moving_scipy.py prints it; the per-trajectory figures are in the golden file).
GAP_MOVING_AT_DEFAULT = 1.263e-2
GAP_MOVING_CASE = (3, "ragged", 0)

batch_of = AO.batch_of


def _line(b, t, j, rng, traj_start):
    so, r = b["seg_offsets"], b["r"]
    s0, s1 = int(so[t]), int(so[t + 1])
    p = b["waypoints"][s0 + t + j] + rng.uniform(-0.2, 0.2, size=3) * (1.0, 1.0, 0.5)
    F = float(np.sum(b["times"][s0:s1]))
    Do = 0.4 * F * rng.uniform(0.9, 1.1)
    ang = rng.uniform(0.0, 2.0 * np.pi)
    vel = rng.uniform(0.7, 1.3) * np.array([np.cos(ang), np.sin(ang), rng.uniform(-0.1, 0.1)])
    c = np.zeros((3, 1, 2 * r))
    c[:, 0, 0] = p - 0.5 * Do * vel
    c[:, 0, 1] = vel
    return np.array([Do]), c, traj_start + float(np.sum(b["times"][s0:s0 + j])) - 0.5 * Do


def obstacles_of(r, kind):
    """The obstacle dict (host arrays, as Context.moving_penalty_host takes it) of batch_of(r, kind): set t = the two tracks of trajectory t."""
    b = batch_of(r, kind)
    n = b["seg_offsets"].size - 1
    rng = np.random.default_rng(OBSTACLE_SEED[r])
    traj_start = rng.uniform(0.0, 0.5, size=n)
    tracks = []
    for t in range(n):
        M = int(b["seg_offsets"][t + 1] - b["seg_offsets"][t])
        j = max(M // 2, 1) if M > 1 else 0
        tracks.append(_line(b, t, j, rng, traj_start[t]))
        tracks.append(_line(b, t, max(j - 1, 0), rng, traj_start[t]))
    return dict(MP._pack(r, tracks), radius=rng.uniform(0.0, 0.2, size=len(tracks)), set_offsets=np.arange(0, 2 * n + 1, 2, dtype=np.int32),
                traj_set=np.arange(n, dtype=np.int32), traj_start=traj_start)


class MovingProblem(AO.AttitudeProblem):
    """f of AttitudeProblem + Phi_moving; grad() is R.Problem.grad, fed with the summed partial gradients of all four penalties."""

    def __init__(self, oracle, r, wp, T, bc, tracks, start, moving=None, **kw):
        super().__init__(oracle, r, wp, T, bc, **kw)
        self.tracks, self.start = tracks, float(start)
        self.mp = dict(MOVING, **(moving or {}))

    def parts(self, p, T):
        q = super().parts(p, T)
        mov = MP.trajectory(self.r, T, q["c"], self.start, self.tracks, **self.mp)
        phi_mov = float(mov["phi"])
        lim = dict(q["lim"])     # (grad() adds lim and clr: the moving term rides on lim's two gradients, as the attitude term does)
        lim["grad_coeff"] = np.asarray(lim["grad_coeff"], dtype=np.float64) + mov["grad_coeff"].astype(np.float64).ravel()
        lim["grad_times"] = np.asarray(lim["grad_times"], dtype=np.float64) + mov["grad_times"].astype(np.float64)
        return dict(q, f=q["f"] + phi_mov, phi=q["phi"] + phi_mov, lim=lim, mov=mov, phi_mov=phi_mov, min_gap=float(mov["min_gap"]),
                    nearest=int(mov["nearest"]))


def problem_of(oracle, r, kind, t, **kw):
    wp, T, bc = R.split(batch_of(r, kind), t)
    obs = obstacles_of(r, kind)
    tracks = MP.obstacle_tracks(r, obs)[int(obs["set_offsets"][t]):int(obs["set_offsets"][t + 1])]
    return MovingProblem(oracle, r, wp, T, bc, tracks, obs["traj_start"][t], **kw)


def iterate(prob, max_iters=DEFAULT_MAX_ITERS, **params):
    return AO.iterate(prob, max_iters, **params)
