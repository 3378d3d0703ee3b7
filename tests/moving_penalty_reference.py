"""Reference of the moving-obstacle penalty (uavqp_moving_penalty_device, include/uavqp.h) in numpy longdouble, written from the
definition as plain loops over segments, samples and obstacles -- not as the kernel's rounds: the suffix sum of the duration gradient is
the sum the header states, taken per segment.

    trajectory(r, T, C, S, tracks, **params)    one trajectory against a list of tracks: Phi, the three gradients, min_gap, nearest, margins
    penalty(r, seg_offsets, times, coeff, obstacles, ...)   a batch in the C-ABI layout, obstacles as the dict of Context.moving_penalty_host
    batch(...), per_trajectory_obstacles(...), one_set_obstacles(...)     what the tests fly

The obstacle's position is the rule of the swarm penalty (swarm_reference.locate: waiting, the segment rule, arrived with the cap).
Margins (what a finite-difference test must stay away from):
    hold_margin   smallest distance in time of any (sample, obstacle) from the obstacle's departure and arrival
    knot_margin   smallest distance in time of any moving obstacle sample from the instant at which the segment rule changes segment
"""
import numpy as np

import swarm_reference as S

LD = np.longdouble
DEFAULTS = dict(samples_per_seg=8, d_safe=1.0, downwash=1.0, weight=1e3)


def knots(T, start, round_clock=True):
    """The clock knots: the DOUBLES K_0 = start, K_{m+1} = fl(K_m + T_m).  round_clock False: the same sums unrounded, in longdouble
    (what a finite-difference test of Phi needs: a step of 1e-6 T must not drown in the rounding of the clock)."""
    cast = np.float64 if round_clock else LD
    K = [cast(start)]
    for Tm in T:
        K.append(cast(K[-1] + cast(Tm)))
    return K


def trajectory(r, T, C, start, tracks, grads=True, **params):
    """T [M] durations, C [3][M][2r] coefficients, start: the departure; tracks: list of (index, T_o, C_o [3][Mo][2r], start_o, radius_o)."""
    p = dict(DEFAULTS, **params)
    round_clock = bool(p.pop("round_clock", True))
    K, d_safe, dw, w = int(p["samples_per_seg"]), LD(p["d_safe"]), LD(p["downwash"]), LD(p["weight"])
    M, nc = len(T), 2 * r
    Dg = np.array([1, 1, 1 / (dw * dw)], dtype=LD)
    kn = knots(T, start, round_clock)
    phi_seg = np.zeros(M, dtype=LD)
    local = np.zeros(M, dtype=LD)          # sum_s om_s tau_s (G . v + Gt)
    Q = np.zeros(M, dtype=LD)
    g_c = np.zeros((3, M, nc), dtype=LD)
    min_gap, nearest = np.inf, -1
    hold_margin = knot_margin = np.inf
    states = set()
    for m in range(M):
        Tm = LD(T[m])
        for s in range(K + 1):
            tau = LD(s) / LD(K)
            t = tau * Tm
            t_abs = tau * Tm + LD(kn[m])
            if round_clock:
                t_abs = LD(np.float64(t_abs))
            om = LD(0.5) if s in (0, K) else LD(1)
            q = np.array([S.horner(C[ax][m], t, 0) for ax in range(3)], dtype=LD)
            G, Gt, x3 = np.zeros(3, dtype=LD), LD(0), LD(0)
            for (o, To, Co, so, rad) in tracks:
                if len(To) < 1:
                    continue
                seg, tl, state, km, hm = S.locate(To, so, t_abs)
                hold_margin, knot_margin = min(hold_margin, hm), min(knot_margin, km)
                states.add(state)
                pos = np.array([S.horner(Co[ax][seg], tl, 0) for ax in range(3)], dtype=LD)
                delta = q - pos
                d2 = delta[0] ** 2 + delta[1] ** 2 + (delta[2] / dw) ** 2
                gap = float(np.sqrt(d2) - LD(rad))
                if gap < min_gap:          # (obstacles ascend inside a sample; an equal gap at a later sample keeps the smaller index below)
                    min_gap, nearest = gap, o
                elif gap == min_gap and o < nearest:
                    nearest = o
                Do = d_safe + LD(rad)
                x = max(LD(0), 1 - d2 / (Do * Do))
                if x > 0:
                    e = -6 * w * x * x / (Do * Do) * Dg * delta
                    G += e
                    x3 += x ** 3
                    if state == S.MOVING:
                        vel = np.array([S.horner(Co[ax][seg], tl, 1) for ax in range(3)], dtype=LD)
                        Gt -= np.dot(e, vel)
            phi_seg[m] += om * w * x3
            if not grads or not (np.any(G) or Gt != 0):
                continue
            v = np.array([S.horner(C[ax][m], t, 1) for ax in range(3)], dtype=LD)
            local[m] += om * tau * (np.dot(G, v) + Gt)
            Q[m] += om * Gt
            for ax in range(3):
                for n in range(nc):
                    g_c[ax][m][n] += om * G[ax] * t ** n
    h = np.array([LD(T[m]) / LD(K) for m in range(M)], dtype=LD)
    Phi_seg = h * phi_seg
    W = h * Q
    g_t = np.array([phi_seg[l] / LD(K) + h[l] * local[l] + sum(W[m] for m in range(l + 1, M)) for l in range(M)], dtype=LD)
    return dict(phi=np.sum(Phi_seg), grad_coeff=g_c * h[None, :, None], grad_times=g_t, grad_start=np.sum(W), W=W, min_gap=min_gap,
                nearest=nearest, hold_margin=hold_margin, knot_margin=knot_margin, states=states)


def obstacle_tracks(r, obstacles):
    """The tracks of an obstacle dict (host arrays) as a list of (index, T_o, C_o, start_o, radius_o)."""
    To = np.asarray(obstacles["times"], dtype=np.float64).ravel()
    uni = int(obstacles.get("uniform_segments", 0))
    oso = np.arange(0, To.size + 1, uni) if uni > 0 else np.asarray(obstacles["seg_offsets"])
    n_obs = oso.size - 1
    start = obstacles.get("start")
    radius = obstacles.get("radius")
    out = []
    for o in range(n_obs):
        T_o, C_o = S.split(r, oso, To, np.asarray(obstacles["coeff"], dtype=np.float64).ravel(), o)
        out.append((o, T_o, C_o, 0.0 if start is None else float(start[o]), 0.0 if radius is None else float(radius[o])))
    return out


def penalty(r, seg_offsets, times, coeff, obstacles, status=None, grads=True, **params):
    """The batch in the C-ABI layout.  Returns dict(phi [n_traj], grad_coeff, grad_times, grad_start [n_traj], min_gap [n_traj], nearest
    [n_traj] as arrays in the layout of the C ABI; W [sum M]: (T_m / K) Q_m per segment; hold_margin, knot_margin, states over the batch)."""
    so = np.asarray(seg_offsets)
    n_traj = so.size - 1
    tracks = obstacle_tracks(r, obstacles)
    set_off = obstacles.get("set_offsets")
    set_off = np.array([0, len(tracks)]) if set_off is None else np.asarray(set_off)
    traj_set = obstacles.get("traj_set")
    traj_set = np.zeros(n_traj, dtype=np.int64) if traj_set is None else np.asarray(traj_set)
    traj_start = obstacles.get("traj_start")
    traj_start = np.zeros(n_traj) if traj_start is None else np.asarray(traj_start)
    nc = 2 * r
    out = dict(phi=np.zeros(n_traj), grad_coeff=np.zeros(len(coeff)), grad_times=np.zeros(len(times)), grad_start=np.zeros(n_traj),
               W=np.zeros(len(times)), min_gap=np.full(n_traj, np.inf), nearest=np.full(n_traj, -1, dtype=np.int32), hold_margin=np.inf,
               knot_margin=np.inf, states=set(), has_set=np.zeros(n_traj, dtype=bool))
    for b in range(n_traj):
        s0, s1 = int(so[b]), int(so[b + 1])
        k = int(traj_set[b])
        if s1 - s0 < 1 or k < 0 or (status is not None and int(status[b]) != 1):
            continue
        mine = tracks[int(set_off[k]):int(set_off[k + 1])]
        if not mine:
            continue
        out["has_set"][b] = True
        T, C = S.split(r, so, times, coeff, b)
        q = trajectory(r, T, C, traj_start[b], mine, grads=grads, **params)
        out["phi"][b] = float(q["phi"])
        out["grad_coeff"][3 * nc * s0:3 * nc * s1] = q["grad_coeff"].astype(np.float64).ravel()
        out["grad_times"][s0:s1] = q["grad_times"].astype(np.float64)
        out["W"][s0:s1] = q["W"].astype(np.float64)
        out["grad_start"][b] = float(q["grad_start"])
        out["min_gap"][b], out["nearest"][b] = q["min_gap"], q["nearest"]
        out["hold_margin"], out["knot_margin"] = min(out["hold_margin"], q["hold_margin"]), min(out["knot_margin"], q["knot_margin"])
        out["states"] |= q["states"]
    return out


# ---------------------------------------------------------------------------------------------------
# What the tests fly
# ---------------------------------------------------------------------------------------------------
def batch(r, Ms, seed, shared=False):
    """Trajectories of M segments each: a random walk of about 1 m per waypoint, durations 0.5 s +- 25 %, zero boundary derivatives.
    shared: every trajectory is the first one's path of its own length, moved by up to 0.1 m (one set of obstacles then meets them all)."""
    rng = np.random.default_rng(seed)
    n = len(Ms)
    so = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32)
    base = np.cumsum(np.vstack([rng.uniform(-1.0, 1.0, size=(1, 3)), rng.uniform(-1.0, 1.0, size=(max(Ms), 3)) * (1.0, 1.0, 0.3)]), axis=0)
    wp, T = [], []
    for M in Ms:
        if shared:
            w = base[:M + 1] + rng.uniform(-0.1, 0.1, size=(M + 1, 3))
        else:
            w = np.cumsum(np.vstack([rng.uniform(-3.0, 3.0, size=(1, 3)), rng.uniform(-1.0, 1.0, size=(M, 3)) * (1.0, 1.0, 0.3)]), axis=0)
        wp.append(w)
        T.append(0.5 * rng.uniform(0.75, 1.25, size=M))
    return dict(r=r, M=0, seg_offsets=so, waypoints=np.vstack(wp), times=np.concatenate(T), bc=np.zeros((n, 2, r - 1, 3)))


def _track_alongside(b, t, solve, offset, traj_start):
    """the trajectory's own waypoints moved by `offset`, its durations, a start 0.05 s later: it flies alongside"""
    so, r = b["seg_offsets"], b["r"]
    s0, s1 = int(so[t]), int(so[t + 1])
    w = b["waypoints"][s0 + t:s1 + t + 1] + np.asarray(offset)
    T = b["times"][s0:s1].copy()
    return T, solve(r, w, np.zeros((2, r - 1, 3)), T), traj_start + 0.05


def _track_line(b, t, rng, traj_start):
    """ONE segment at constant velocity (higher coefficients zero) through a waypoint of the trajectory at the time the trajectory is
    there; 0.4 of the flight long, so that on a long trajectory it waits first and has arrived at the end"""
    so, r = b["seg_offsets"], b["r"]
    s0, s1 = int(so[t]), int(so[t + 1])
    M = s1 - s0
    j = M // 2
    p = b["waypoints"][s0 + t + j] + rng.uniform(-0.2, 0.2, size=3)
    F = float(np.sum(b["times"][s0:s1]))
    Do = max(0.4 * F, 0.3) * rng.uniform(0.9, 1.1)
    vel = rng.uniform(-1.5, 1.5, size=3) * (1.0, 1.0, 0.2)
    c = np.zeros((3, 1, 2 * r))
    c[:, 0, 0] = p - 0.5 * Do * vel
    c[:, 0, 1] = vel
    return np.array([Do]), c, traj_start + float(np.sum(b["times"][s0:s0 + j])) - 0.5 * Do


def _track_five(b, t, solve, rng, traj_start):
    """FIVE segments from rest to rest across the trajectory's path near its first third"""
    so, r = b["seg_offsets"], b["r"]
    s0, s1 = int(so[t]), int(so[t + 1])
    M = s1 - s0
    j = max(M // 3, 0)
    p = b["waypoints"][s0 + t + j]
    F = float(np.sum(b["times"][s0:s1]))
    d = rng.uniform(-1.0, 1.0, size=3) * (1.0, 1.0, 0.2)
    d /= np.linalg.norm(d)
    w = p + np.linspace(-1.2, 1.2, 6)[:, None] * d + rng.uniform(-0.1, 0.1, size=(6, 3))
    T = max(0.12 * F, 0.1) * rng.uniform(0.8, 1.2, size=5)
    return T, solve(r, w, np.zeros((2, r - 1, 3)), T), traj_start + float(np.sum(b["times"][s0:s0 + j])) - 0.5 * float(np.sum(T))


def _pack(r, tracks):
    Ts, Cs, starts = zip(*tracks) if tracks else ((), (), ())
    oso = np.concatenate([[0], np.cumsum([len(T) for T in Ts])]).astype(np.int32)
    coeff = np.concatenate([np.asarray(C, dtype=np.float64).reshape(3, len(T), 2 * r).ravel() for T, C in zip(Ts, Cs)]) if tracks else np.zeros(0)
    return dict(seg_offsets=oso, times=np.concatenate(Ts) if tracks else np.zeros(0), coeff=coeff, start=np.array(starts, dtype=np.float64))


SET_SIZES = (1, 3, 0)       # the set of trajectory t has SET_SIZES[t % 3] obstacles
ALONGSIDE = (0.3, -0.25, 0.1)   # |.| = 0.40 m: well inside D_o >= d_safe = 1 m


def per_trajectory_obstacles(b, solve, seed, none_at=4):
    """One set per trajectory, of SET_SIZES[t % 3] obstacles: the first flies alongside the trajectory, the second is a one-segment line,
    the third a five-segment track, both across its path.  traj_set explicit (the identity) with a -1 at `none_at`; radii given;
    departures of the trajectories spread over [-0.4, 0.6]."""
    rng = np.random.default_rng(seed)
    n = b["seg_offsets"].size - 1
    traj_start = rng.uniform(-0.4, 0.6, size=n)
    tracks, set_off = [], [0]
    for t in range(n):
        size = SET_SIZES[t % 3]
        if size >= 1:
            tracks.append(_track_alongside(b, t, solve, ALONGSIDE, traj_start[t]))
        if size >= 2:
            tracks.append(_track_line(b, t, rng, traj_start[t]))
        if size >= 3:
            tracks.append(_track_five(b, t, solve, rng, traj_start[t]))
        set_off.append(len(tracks))
    traj_set = np.arange(n, dtype=np.int32)
    traj_set[none_at] = -1
    return dict(_pack(b["r"], tracks), radius=rng.uniform(0.0, 0.3, size=len(tracks)), set_offsets=np.array(set_off, dtype=np.int32),
                traj_set=traj_set, traj_start=traj_start)


def one_set_obstacles(b, solve, seed):
    """ONE set of three obstacles for a `shared` batch, traj_set and set_offsets absent (NULL), no radii, no departures of the trajectories:
    alongside the LONGEST trajectory, a line and a five-segment track across it."""
    rng = np.random.default_rng(seed)
    t = int(np.argmax(np.diff(b["seg_offsets"])))
    tracks = [_track_alongside(b, t, solve, ALONGSIDE, 0.0), _track_line(b, t, rng, 0.0), _track_five(b, t, solve, rng, 0.0)]
    return _pack(b["r"], tracks)
