"""Reference of the swarm separation penalty (uavqp_swarm_penalty_device, include/uavqp.h) in numpy longdouble, written from the
definition as plain loops over clock samples and pairs of vehicles -- not as the kernel's phases: positions are evaluated where a pair
needs them, forces are added to both vehicles of a pair as the pair is met, and the duration gradient is the sum the header states.

    swarm(r, Ts, Cs, starts, live, **params)      one swarm: Phi, the three gradients, min_sep and the margins of its samples
    penalty(r, seg_offsets, times, coeff, ...)    a batch in the C-ABI layout: the same per swarm, assembled into the C-ABI outputs
    scene(...)                                    vehicles laid through a common region, staggered departures (what the tests fly)

Margins (what a finite-difference test must stay away from, and what the tests assert before they difference anything):
    knot_margin   smallest distance in time of any moving sample from the instant at which the segment rule changes segment
    hold_margin   smallest distance in time of any sample from its vehicle's departure and from its arrival
    rho_gap       smallest |rho2 - 1| over the pairs that are penalised (x > 0); rho_gap_all over every pair
"""
import numpy as np

LD = np.longdouble
DEFAULTS = dict(n_samples=64, clock_start=0.0, dt=0.1, d_safe=1.0, downwash=1.0, weight=1e3)
SLACK = 1e-4          # the segment rule's (qp_poly.h: poly_past_segment)
MOVING, WAITING, ARRIVED = 0, 1, 2


def clock(k, clock_start, dt):
    """t_k: the double nearest to clock_start + k dt."""
    return LD(np.float64(LD(clock_start) + LD(k) * LD(dt)))


def locate(T, start, t):
    """(segment, local time, state, knot margin, hold margin) of a vehicle with durations T at clock time t."""
    M = len(T)
    u = t - LD(start)
    if u < 0:
        return 0, LD(0), WAITING, np.inf, float(-u)
    idx, tl = 0, u
    while idx < M and tl > LD(np.float64(T[idx]) + np.float64(SLACK)):
        tl -= LD(T[idx])
        idx += 1
    if idx == M:
        # (the walk left the last segment: beyond T_{M-1} by more than the slack)
        return M - 1, LD(T[M - 1]), ARRIVED, np.inf, min(float(tl), float(u))     # tl: the time since the arrival
    knot = np.inf
    if idx > 0:
        knot = min(knot, float(tl) - SLACK)                      # how far behind the previous segment's threshold
    hold = float(u)                                              # since the departure
    if idx < M - 1:
        knot = min(knot, float(LD(T[idx]) + LD(SLACK) - tl))     # how far before this segment's threshold
        return idx, tl, MOVING, knot, hold
    hold = min(hold, abs(float(LD(T[M - 1]) - tl)))              # from the arrival
    if tl >= LD(T[M - 1]):
        return M - 1, LD(T[M - 1]), ARRIVED, np.inf, hold
    return idx, tl, MOVING, knot, hold


def horner(c, t, deriv):
    """deriv-th derivative at t of the polynomial with ascending coefficients c (longdouble)."""
    v = LD(0)
    for n in range(len(c) - 1, deriv - 1, -1):
        f = LD(1)
        for j in range(deriv):
            f *= n - j
        v = v * t + f * LD(c[n])
    return v


def swarm(r, Ts, Cs, starts, live=None, grads=True, **params):
    """One swarm.  Ts[i]: durations [M_i]; Cs[i]: coefficients [3][M_i][2r]; starts[i]; live[i]: takes part (solved and M >= 1)."""
    p = dict(DEFAULTS, **params)
    N, dt, d_safe, dw, w = int(p["n_samples"]), LD(p["dt"]), LD(p["d_safe"]), LD(p["downwash"]), LD(p["weight"])
    A, nc = len(Ts), 2 * r
    live = [len(Ts[i]) >= 1 and (live is None or bool(live[i])) for i in range(A)]
    D = np.array([1, 1, 1 / (dw * dw)], dtype=LD)
    phi = LD(0)
    g_c = [np.zeros((3, len(Ts[i]), nc), dtype=LD) for i in range(A)]
    Wm = [np.zeros(len(Ts[i]), dtype=LD) for i in range(A)]
    P = np.zeros(A, dtype=LD)
    min_rho2 = np.full(A, np.inf, dtype=LD)
    knot_margin = hold_margin = rho_gap = rho_gap_all = np.inf
    states = set()
    for k in range(N + 1):
        t = clock(k, p["clock_start"], p["dt"])
        om = LD(0.5) if k in (0, N) else LD(1)
        where = {}
        for i in range(A):
            if not live[i]:
                continue
            seg, tl, state, km, hm = locate(Ts[i], starts[i], t)
            q = np.array([horner(Cs[i][ax][seg], tl, 0) for ax in range(3)], dtype=LD)
            where[i] = (seg, tl, state, q)
            knot_margin, hold_margin = min(knot_margin, km), min(hold_margin, hm)
            states.add(state)
        # every unordered pair once: vehicle i against its partners j > i (the partners of one i as one array), the pair's force added
        # to i and taken from j
        ids = sorted(where)
        Q = np.array([where[i][3] for i in ids], dtype=LD).reshape(len(ids), 3)
        Gs = np.zeros((len(ids), 3), dtype=LD)
        for a in range(len(ids) - 1):
            delta = Q[a] - Q[a + 1:]
            rho2 = (delta[:, 0] ** 2 + delta[:, 1] ** 2 + (delta[:, 2] / dw) ** 2) / (d_safe * d_safe)
            min_rho2[ids[a]] = min(min_rho2[ids[a]], np.min(rho2))
            min_rho2[ids[a + 1:]] = np.minimum(min_rho2[ids[a + 1:]], rho2)
            rho_gap_all = min(rho_gap_all, float(np.min(np.abs(rho2 - 1))))
            x = np.maximum(1 - rho2, 0)
            if not np.any(x > 0):
                continue
            rho_gap = min(rho_gap, float(np.min(x[x > 0])))
            phi += dt * om * w * np.sum(x ** 3)
            e = (-6 * w * x * x / (d_safe * d_safe))[:, None] * D * delta
            Gs[a] += np.sum(e, axis=0)
            Gs[a + 1:] -= e
        G = {i: Gs[a] for a, i in enumerate(ids)}
        if not grads:
            continue
        for i, (seg, tl, state, _) in where.items():
            if not np.any(G[i]):
                continue
            for ax in range(3):
                for n in range(nc):
                    g_c[i][ax][seg][n] += dt * om * G[i][ax] * tl ** n
            Gv = sum(G[i][ax] * horner(Cs[i][ax][seg], tl, 1) for ax in range(3))
            if state == MOVING:
                Wm[i][seg] += om * Gv
            elif state == ARRIVED:
                P[i] += om * Gv
    g_t = []
    for i in range(A):
        M = len(Ts[i])
        gt = np.zeros(M, dtype=LD)
        for l in range(M):
            gt[l] = -dt * sum(Wm[i][m] for m in range(l + 1, M)) + (dt * P[i] if l == M - 1 else 0)
        g_t.append(gt)
    g_s = np.array([-dt * sum(Wm[i]) for i in range(A)], dtype=LD)
    min_sep = np.array([float(d_safe * np.sqrt(min_rho2[i])) if live[i] and np.isfinite(min_rho2[i]) else np.inf for i in range(A)])
    return dict(phi=phi, grad_coeff=g_c, grad_times=g_t, grad_start=g_s, min_sep=min_sep, knot_margin=knot_margin, hold_margin=hold_margin,
                rho_gap=rho_gap, rho_gap_all=rho_gap_all, states=states)


def split(r, seg_offsets, times, coeff, b):
    """(durations, coefficients [3][M][2r]) of trajectory b of a batch in the C-ABI layout."""
    s0, s1 = int(seg_offsets[b]), int(seg_offsets[b + 1])
    nc = 2 * r
    return np.asarray(times[s0:s1]), np.asarray(coeff[3 * nc * s0:3 * nc * s1]).reshape(3, s1 - s0, nc)


def penalty(r, seg_offsets, times, coeff, group_offsets=None, start=None, status=None, grads=True, **params):
    """The batch in the C-ABI layout.  Returns dict(phi [n_groups], grad_coeff, grad_times, grad_start, min_sep as float64 arrays in the
    layout of the C ABI; knot_margin, hold_margin, rho_gap, rho_gap_all over the batch; states: the hold states that were sampled;
    per_swarm: the dicts of swarm())."""
    so = np.asarray(seg_offsets)
    n_traj = so.size - 1
    go = np.array([0, n_traj]) if group_offsets is None else np.asarray(group_offsets)
    start = np.zeros(n_traj) if start is None else np.asarray(start)
    out = dict(phi=np.zeros(go.size - 1), grad_coeff=np.zeros(len(coeff)), grad_times=np.zeros(len(times)), grad_start=np.zeros(n_traj),
               min_sep=np.full(n_traj, np.inf), knot_margin=np.inf, hold_margin=np.inf, rho_gap=np.inf, rho_gap_all=np.inf, states=set(),
               per_swarm=[])
    nc = 2 * r
    for g in range(go.size - 1):
        bs = list(range(int(go[g]), int(go[g + 1])))
        parts = [split(r, so, times, coeff, b) for b in bs]
        live = [status is None or int(status[b]) == 1 for b in bs]
        q = swarm(r, [pt[0] for pt in parts], [pt[1] for pt in parts], [start[b] for b in bs], live, grads=grads, **params)
        out["per_swarm"].append(q)
        out["phi"][g] = float(q["phi"])
        for i, b in enumerate(bs):
            s0, s1 = int(so[b]), int(so[b + 1])
            out["grad_coeff"][3 * nc * s0:3 * nc * s1] = q["grad_coeff"][i].astype(np.float64).ravel()
            out["grad_times"][s0:s1] = q["grad_times"][i].astype(np.float64)
            out["grad_start"][b] = float(q["grad_start"][i])
            out["min_sep"][b] = q["min_sep"][i]
        for key in ("knot_margin", "hold_margin", "rho_gap", "rho_gap_all"):
            out[key] = min(out[key], q[key])
        out["states"] |= q["states"]
    return out


def scene(rng, Ms, centre=(0.0, 0.0, 1.0), radius=1.6, flight=2.0, start_span=(-0.3, 0.5), spread=0.0):
    """Vehicles of one swarm laid through a common region: vehicle i starts on a circle of `radius` around `centre` and ends opposite,
    its interior waypoints on the chord with some noise, so that the paths cross near the centre at about the same time; the
    durations add up to about `flight` seconds and the departures are staggered over start_span.  spread > 0 moves vehicle i by
    i * spread along x: a swarm whose vehicles never come near one another.
    Returns (waypoints list of [M_i + 1][3], durations list of [M_i], starts [A])."""
    A = len(Ms)
    wps, Ts = [], []
    phase = rng.uniform(0.0, 2.0 * np.pi)
    for i, M in enumerate(Ms):
        ang = phase + 2.0 * np.pi * i / A + rng.uniform(-0.2, 0.2)
        p0 = np.array(centre) + radius * np.array([np.cos(ang), np.sin(ang), 0.25 * rng.uniform(-1.0, 1.0)])
        p1 = 2.0 * np.array(centre) - p0 + rng.uniform(-0.3, 0.3, size=3)
        s = np.linspace(0.0, 1.0, M + 1)[:, None]
        wp = (1.0 - s) * p0 + s * p1
        wp[1:M] += rng.uniform(-0.15, 0.15, size=(M - 1, 3))
        wp[:, 0] += i * spread
        wps.append(wp)
        Ts.append(flight / M * rng.uniform(0.8, 1.2, size=M))
    return wps, Ts, rng.uniform(start_span[0], start_span[1], size=A)
