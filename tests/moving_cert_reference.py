"""CPU reference of uavqp_moving_certificate_* (include/uavqp.h): the method of csrc/qp_moving_cert.h restated in numpy float64 with the
kernel's order of operations (certificate), an independent TRUTH (truth: the definition of the certified curves evaluated with mpmath at
60 digits, the obstacle located in exact arithmetic on the double knots), and the inputs the CPU test
(tests/test_moving_cert_reference.py) qualifies for the GPU test (tests/test_gpu_moving_cert.py).

The certified curves.  Trajectory b departs at S = traj_start[b]; its clock knots are the DOUBLES K_0 = S, K_{m+1} = fl(K_m + T_m).  At local
time s of segment m it is at q_m(s) and the clock shows K_m + s (real arithmetic).  Obstacle o is the curve of the separation certificate
(tests/separation_cert_reference.py) on that clock: segment 0 at local time 0 for t <= K^o_0, segment m at local time t - K^o_m for t in
[K^o_m, K^o_{m+1}], the last segment at its end for t >= K^o_M; pieces are closed (at a knot both values belong to the curve).
    gap_o(t) = sqrt(dx^2 + dy^2 + (dz / downwash)^2) - radius_o   of q(t) - o(t)

The method, n = 2r - 1.  Leaf l of segment m: local time [l, l + 1] T_m / 2^depth, clock ends ta = fma(l 2^-depth, T_m, K_m), tb =
fma((l + 1) 2^-depth, T_m, K_m).  The trajectory over the leaf: envelope_reference.bernstein and depth midpoint splits, guard G_x =
16 (n + 1) 2^-53 S_x.  The obstacle over [ta, tb]: the entry of the separation certificate (SINGLE: the leaf lies in one piece; BOX: the
per-axis [lo, hi] over the pieces it meets) with the guard, the largest over the pieces,
    G^o_x = (64 (n + 1) + 4 n kappa_o) 2^-53 S_x,   kappa_o = max(|K^o_m|, |K^o_{m+1}|, |ta|, |tb|) / T^o_m
and for a held obstacle (waiting, arrived) the separation rule (64 (n + 1) + 2 n kappa) 2^-53 S_x, kappa = max(|K^o_m|, |K^o_{m+1}|) / T^o_m.
A rounded ta (tb) is not trusted: it stands for [t - 2^-52 |t|, t + 2^-52 |t|], which holds the real end (an exact one -- dyadic durations
and departures -- stands for itself); which pieces the leaf meets and whether it lies in one is decided on [ta_lo, tb_hi], a piece met
through the margin alone comes in as its end point and makes the entry a BOX, and where a knot lies in the interval of an end of a leaf
that is not in one piece, that obstacle gives no witness there.
Pair (leaf, o), Gs = G + G^o, w the leaf's coefficients: single, [lo_x, hi_x] = [min_k, max_k] of w_k - b^o_k; box, the interval difference
with the box of w; lo -= Gs, hi += Gs, g_x = max(0, lo_x, -hi_x),
    L = max(0, sqrt(g_x^2 + g_y^2 + (g_z / downwash)^2) - R) - radius_o,         R = 16 2^-53 sum_x max(|lo_x|, |hi_x|)
    U = s(d) + sqrt(3) max_x Gs_x + 16 2^-53 (|d_x| + |d_y| + |d_z|) - radius_o    d = the difference of the end coefficients at a witness
Per segment: lower = min L, upper = min U; ties: the smaller obstacle, then the smaller leaf / witness.
ALLOWANCE of a pair on a leaf: sqrt(3) max_x Gs_x + R, within which two evaluations of these formulas agree."""
import functools
from fractions import Fraction

import numpy as np

import clearance_cert_reference as CC
import envelope_reference as E
import moving_penalty_reference as MP
import separation_cert_reference as SC
import swarm_reference as SW

EPS = 2.0 ** -53
SQRT3 = 1.7320508075688772
CERTIFIED, VIOLATED = 1, 2
SOLVED = 1
SINGLE, BOX = SC.SINGLE, SC.BOX
MOVING, WAITING, ARRIVED, STRADDLING = 0, 1, 2, 3
DEFAULTS = dict(depth=3, downwash=1.0, d_req=1.0)
OUT = ("gap", "where", "peak", "seg_verdict", "verdict")
NONE = np.array([-1, 0, -1, 0], dtype=np.int32)


def leaf_clock(K, T, depth):
    """(ta_l = fma(l 2^-depth, T, K), l = 0..2^depth, and whether each IS l 2^-depth T + K); tb_l is ta_{l+1}: the same operation on the same
    numbers"""
    n = 1 << depth
    if not (np.isfinite(K) and np.isfinite(T)):      # (what float64 arithmetic gives: NaN, or an infinite clock; never exact)
        with np.errstate(all="ignore"):
            return np.array([np.float64(l / n) * np.float64(T) + np.float64(K) for l in range(n + 1)]), np.zeros(n + 1, dtype=bool)
    real = [Fraction(l, n) * Fraction(float(T)) + Fraction(float(K)) for l in range(n + 1)]
    tw = np.array([float(x) for x in real])
    return tw, np.array([Fraction(float(t)) == x for t, x in zip(tw, real)])


def entries(T, C, start, tw, exact, force_box=False):
    """The entries of one obstacle (durations T [M], coefficients C [3][M][nc]) on the leaves of tw -- separation_cert_reference.entries with
    the guard of this certificate and its distrust of a rounded end: an inexact ta (tb) stands for [t - 2^-52 |t|, t + 2^-52 |t|], the
    pieces a leaf meets and whether it lies in one are decided on [ta_lo, tb_hi], the ratios on [ta, tb].  bad [NL]: a piece the leaf
    meets has a duration that is not > 0; amb_l / amb_r [NL]: a knot lies where the real left / right end can, and the leaf is not in
    one piece -- no witness there."""
    M, nc = len(T), C.shape[2]
    ta, tb = tw[:-1], tw[1:]
    NL = ta.size
    tmag = np.fmax(np.abs(ta), np.abs(tb))
    ma, mb = np.where(exact[:-1], 0.0, 2.0 * EPS * np.abs(ta)), np.where(exact[1:], 0.0, 2.0 * EPS * np.abs(tb))
    ta_lo, ta_hi, tb_lo, tb_hi = ta - ma, ta + ma, tb - mb, tb + mb
    amb_l, amb_r = np.zeros(NL, dtype=bool), np.zeros(NL, dtype=bool)
    K = SC.knots(T, start)
    e = dict(kind=np.full(NL, BOX), coef=np.zeros((NL, 3, nc)), lo=np.zeros((NL, 3)), hi=np.zeros((NL, 3)), G=np.zeros((NL, 3)),
             left=np.zeros((NL, 3)), right=np.zeros((NL, 3)), K=K, state=np.zeros(NL, dtype=int), bad=np.zeros(NL, dtype=bool))
    pieces = np.zeros(NL, dtype=int)

    def add(mask, m, lam1, lam2, held):
        if not mask.any():
            return
        with np.errstate(all="ignore"):
            Tm = np.float64(T[m])
            kk = max(abs(K[m]), abs(K[m + 1]))
            kappa = np.full(int(mask.sum()), kk / Tm) if held else 2.0 * (np.fmax(kk, tmag[mask]) / Tm)
            b, S = E.bernstein(C[:, m, :], np.full(3, T[m]), 0)
            first = pieces[mask] == 0
            e["bad"][mask] |= not (Tm > 0.0)
            for ax in range(3):
                g = (64.0 * nc + 2.0 * (nc - 1) * kappa) * EPS * S[ax]
                w = SC.restrict(np.repeat(b[ax][None, :], int(mask.sum()), axis=0), lam1, lam2)
                l, u = w.min(axis=1), w.max(axis=1)
                e["lo"][mask, ax] = np.where(first, l, np.fmin(e["lo"][mask, ax], l))
                e["hi"][mask, ax] = np.where(first, u, np.fmax(e["hi"][mask, ax], u))
                G = e["G"][mask, ax]
                e["G"][mask, ax] = np.where(first | (g > G) | np.isnan(g), g, G)
                e["left"][mask, ax] = np.where(first, w[:, 0], e["left"][mask, ax])
                e["right"][mask, ax] = w[:, -1]
                e["coef"][mask, ax] = w
        pieces[mask] += 1

    with np.errstate(all="ignore"):
        waiting = tb_hi <= K[0]
        n = int(waiting.sum())
        add(waiting, 0, np.zeros(n), np.zeros(n), True)
        done = waiting.copy()
        for m in range(M):
            walked = ~waiting & (K[m] <= tb_hi)
            for k in (K[m], K[m + 1]):
                amb_l |= walked & ~exact[:-1] & (k >= ta_lo) & (k <= ta_hi)
                amb_r |= walked & ~exact[1:] & (k >= tb_lo) & (k <= tb_hi)
            touch = ~done & (K[m] <= tb_hi) & ((K[m + 1] > ta_lo) | ((K[m + 1] == ta_lo) & (m < M - 1)))      # (K_M = ta: arrived)
            inside = touch & (K[m] <= ta_lo) & (tb_hi <= K[m + 1])
            pieces[inside] = 0
            la, lb = np.fmax(ta[touch] - K[m], 0.0), np.fmin(tb[touch] - K[m], T[m])
            add(touch, m, SC.ratio(lb / np.float64(T[m])), SC.ratio(la / lb), False)
            done |= inside
        arrived = pieces == 0
        n = int(arrived.sum())
        add(arrived, M - 1, np.ones(n), np.ones(n), True)
    single = waiting | (done & ~waiting) | arrived
    e["kind"] = np.where(single & (not force_box), SINGLE, BOX)
    e["amb_l"], e["amb_r"] = amb_l & ~single, amb_r & ~single
    e["state"] = np.where(waiting, WAITING, np.where(arrived, ARRIVED, np.where(single, MOVING, STRADDLING)))
    return e


def _norm(d, inv_dw):
    z = d[..., 2] * inv_dw
    return np.sqrt(d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + z * z))


def pair(w, G, e, rad, inv_dw):
    """w [NL][3][nc] the leaves of the segment, G [3] its guard, e the obstacle's entries: (L [NL], U [NL + 1], allowance of L, of U, bad)"""
    nc = w.shape[2]
    with np.errstate(all="ignore"):
        Gs = G[None, :] + e["G"]
        Gmax = np.max(Gs, axis=1)
        Gmax[np.isnan(Gs).any(axis=1)] = np.nan
        bad = bool(np.any(~(Gmax < np.inf)) or np.any(e["bad"]))
        single = e["kind"] == SINGLE
        d = w - e["coef"]
        lo = np.where(single[:, None], d.min(axis=2), w.min(axis=2) - e["hi"]) - Gs
        hi = np.where(single[:, None], d.max(axis=2), w.max(axis=2) - e["lo"]) + Gs
        g = np.fmax(0.0, np.fmax(lo, -hi))
        R = 16.0 * EPS * np.sum(np.fmax(np.abs(lo), np.abs(hi)), axis=1)
        L = np.fmax(0.0, _norm(g, inv_dw) - R) - rad
        pad = SQRT3 * Gmax
        dl, dr = w[:, :, 0] - e["left"], w[-1, :, nc - 1] - e["right"][-1]
        Rl, Rr = 16.0 * EPS * np.sum(np.abs(dl), axis=1), 16.0 * EPS * np.sum(np.abs(dr))
        U = np.concatenate([_norm(dl, inv_dw) + pad + Rl, [_norm(dr, inv_dw) + pad[-1] + Rr]]) - rad
        aU = np.concatenate([pad + Rl, [pad[-1] + Rr]])
        U[np.concatenate([e["amb_l"], e["amb_r"][-1:]])] = np.inf      # no witness where the piece of the instant is open
    return L, U, pad + R, aU, bad


def _tracks(r, obstacles):
    if obstacles.get("times") is None or np.asarray(obstacles["times"]).size == 0:
        return []
    return MP.obstacle_tracks(r, obstacles)


def certificate(r, seg_offsets, times, coeff, obstacles, status=None, force_box=False, **params):
    """The method of qp_moving_cert.h; obstacles: the dict of host arrays Context.moving_certificate_host takes.  Returns the five outputs of
    uavqp_moving_certificate_* and, for the tests: allow [sum M][2] (the allowance of the deciding pair of lower / of upper), runner [sum M][2]
    (how far the runner-up candidate is from the winner), leaf_lower [sum M] (list of arrays [2^depth]: min over the obstacles of L per
    leaf), states (which of moving / waiting / arrived / straddling entries occurred), whole_wait (an obstacle waited through a whole
    flight)."""
    p = dict(DEFAULTS, **params)
    depth, inv_dw, d_req = int(p["depth"]), 1.0 / float(p["downwash"]), float(p["d_req"])
    so = np.asarray(seg_offsets, dtype=np.int64)
    n_traj, tot, nc = so.size - 1, int(so[-1]), 2 * r
    times = np.asarray(times, dtype=np.float64).ravel()
    coeff = np.asarray(coeff, dtype=np.float64).ravel()
    tracks = _tracks(r, obstacles)
    set_off = obstacles.get("set_offsets")
    set_off = np.array([0, len(tracks)]) if set_off is None else np.asarray(set_off)
    traj_set = obstacles.get("traj_set")
    traj_set = np.zeros(n_traj, dtype=np.int64) if traj_set is None else np.asarray(traj_set)
    traj_start = obstacles.get("traj_start")
    traj_start = np.zeros(n_traj) if traj_start is None else np.asarray(traj_start, dtype=np.float64)
    out = dict(gap=np.full((tot, 2), np.inf), where=np.tile(NONE, (tot, 1)), peak=np.full((n_traj, 2), np.inf),
               seg_verdict=np.zeros(tot, dtype=np.int32), verdict=np.zeros(n_traj, dtype=np.int32), allow=np.zeros((tot, 2)),
               runner=np.full((tot, 2), np.inf), leaf_lower=[None] * tot, states=set(), whole_wait=False)
    for b in range(n_traj):
        s0, s1 = int(so[b]), int(so[b + 1])
        if s1 <= s0 or (status is not None and int(status[b]) != SOLVED):
            continue
        k = int(traj_set[b])
        mine = tracks[int(set_off[k]):int(set_off[k + 1])] if k >= 0 else []
        if not mine:
            out["seg_verdict"][s0:s1] = CERTIFIED
            out["verdict"][b] = CERTIFIED
            continue
        T, C = SW.split(r, so, times, coeff, b)
        K = SC.knots(T, traj_start[b])
        waits = {o: True for (o, To, _, _, _) in mine if len(To) >= 1}
        for m in range(s1 - s0):
            seg = s0 + m
            with np.errstate(all="ignore"):
                bb, S = E.bernstein(C[:, m, :], np.full(3, T[m]), 0)
                G = 16.0 * float(nc) * EPS * S
                w = np.stack([CC.leaves_of(bb[ax][None, :], depth)[0] for ax in range(3)], axis=1)      # [NL][3][nc]
            tw, exact = leaf_clock(K[m], T[m], depth)
            # a duration that is not > 0 spoils its segment; a NaN one spoils the clock, and with it every later segment
            bad = not (T[m] > 0.0) or (bool(np.isnan(tw).any()) and any(len(t[1]) >= 1 for t in mine))
            Ls, Us, aL, aU = [], [], {}, {}
            for (o, To, Co, so_, rad) in mine:
                if len(To) < 1:
                    continue
                e = entries(To, Co, so_, tw, exact, force_box)
                out["states"] |= set(e["state"].tolist())
                waits[o] = waits[o] and bool(np.all(e["state"] == WAITING))
                L, U, aL[o], aU[o], pb = pair(w, G, e, rad, inv_dw)
                bad = bad or pb
                Ls.append((o, L))
                Us.append((o, U))
            if bad:
                out["gap"][seg] = np.nan
                continue
            Lv, Lp, Ll, out["runner"][seg, 0] = SC._pick(Ls)
            Uv, Up, Uw, out["runner"][seg, 1] = SC._pick(Us)
            if Lp >= 0:
                out["gap"][seg] = [Lv, Uv]
                out["where"][seg] = [Lp, Ll, Up, Uw]
                out["allow"][seg] = [aL[Lp][Ll], aU[Up][Uw] if Up >= 0 else 0.0]
                out["leaf_lower"][seg] = np.min(np.stack([L for _, L in Ls]), axis=0)
            out["seg_verdict"][seg] = (CERTIFIED if out["gap"][seg, 0] >= d_req else 0) | (VIOLATED if out["gap"][seg, 1] < d_req else 0)
        out["whole_wait"] = out["whole_wait"] or any(waits.values())
        g, bits = out["gap"][s0:s1], out["seg_verdict"][s0:s1]
        if np.isnan(g).any():
            out["peak"][b] = np.nan
        else:
            out["peak"][b] = g.min(axis=0)
            out["verdict"][b] = (np.bitwise_and.reduce(bits) & CERTIFIED) | (np.bitwise_or.reduce(bits) & VIOLATED)
    return out


def state(word):
    return "certified" if int(word) & CERTIFIED else "violated" if int(word) & VIOLATED else "undecided"


def two_allowances_away(ref, d_req):
    """d_req lies more than two allowances from every finite bound: no verdict bit hangs on a rounding"""
    g, a = ref["gap"], ref["allow"]
    return bool(np.all(~np.isfinite(g) | (np.abs(g - d_req) > 2.0 * a)))


def where_comparable(ref):
    """[sum M][2] bool: the runner-up candidate of lower (of upper) is more than two allowances from the winner, so `where` is no tie"""
    return ref["runner"] > 2.0 * ref["allow"]


def tie_fraction(ref):
    """the share of the segments that have bounds whose `where` is a tie, for lower or for upper"""
    have = np.isfinite(ref["gap"]).all(axis=1)
    return float(np.count_nonzero(~where_comparable(ref).all(axis=1) & have)) / max(int(np.count_nonzero(have)), 1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the truth (mpmath, 60 digits): the definition, nothing of the method
# ---------------------------------------------------------------------------------------------------------------------------------------
def truth(r, seg_offsets, times, coeff, obstacles, per_leaf=64, truth_depth=3, downwash=1.0):
    """-> (inst [sum M] list of arrays of gaps (mpf) at the per_leaf 2^truth_depth + 1 instants j T_m / (per_leaf 2^truth_depth) of every
    segment that has obstacles (None otherwise): the min over the obstacles of its set; at(seg, o, num, den): the gap to obstacle o at
    local time (num / den) T of segment seg)."""
    import mpmath
    mp = mpmath.mp
    mp.dps = 60
    so = np.asarray(seg_offsets, dtype=np.int64)
    n_traj, tot = so.size - 1, int(so[-1])
    times = np.asarray(times, dtype=np.float64).ravel()
    coeff = np.asarray(coeff, dtype=np.float64).ravel()
    tracks = _tracks(r, obstacles)
    set_off = obstacles.get("set_offsets")
    set_off = np.array([0, len(tracks)]) if set_off is None else np.asarray(set_off)
    traj_set = obstacles.get("traj_set")
    traj_set = np.zeros(n_traj, dtype=np.int64) if traj_set is None else np.asarray(traj_set)
    traj_start = obstacles.get("traj_start")
    traj_start = np.zeros(n_traj) if traj_start is None else np.asarray(traj_start, dtype=np.float64)
    dw = mp.mpf(float(downwash))
    by_index = {t[0]: t for t in tracks}
    seg_of = {}

    def gap_to(track, q, t):
        _, To, Co, so_, rad = track
        P = SC._positions(mp, To, Co, SC.knots(To, so_), t)
        return min(mp.sqrt((q[0] - c[0]) ** 2 + (q[1] - c[1]) ** 2 + ((q[2] - c[2]) / dw) ** 2) for c in P) - mp.mpf(float(rad))

    def point(seg, num, den):
        T, C, K, m = seg_of[seg]
        s = mp.mpf(float(T[m])) * num / den
        q = []
        for ax in range(3):
            v = mp.mpf(0)
            for c in C[ax][m][::-1]:
                v = v * s + mp.mpf(float(c))
            q.append(v)
        return q, mp.mpf(float(K[m])) + s

    def at(seg, o, num, den):
        q, t = point(seg, num, den)
        return gap_to(by_index[o], q, t)

    inst = [None] * tot
    n_inst = per_leaf << truth_depth
    for b in range(n_traj):
        s0, s1 = int(so[b]), int(so[b + 1])
        k = int(traj_set[b])
        mine = [t for t in (tracks[int(set_off[k]):int(set_off[k + 1])] if k >= 0 else []) if len(t[1]) >= 1]
        if s1 <= s0:
            continue
        T, C = SW.split(r, so, times, coeff, b)
        K = SC.knots(T, traj_start[b])
        for m in range(s1 - s0):
            seg_of[s0 + m] = (T, C, K, m)
            if mine:
                vals = []
                for j in range(n_inst + 1):
                    q, t = point(s0 + m, j, n_inst)
                    vals.append(min(gap_to(tr, q, t) for tr in mine))
                inst[s0 + m] = vals
    return inst, at


def soundness_failures(got, tr, depth, tag=""):
    """leaf lower <= truth at every instant of the leaf (its two ends included) and truth(witness) <= upper, in mpmath arithmetic and WITHOUT
    a tolerance -> list of strings.  got: certificate() at `depth` (leaf_lower) or the device's gap / where (segment lower only)."""
    import mpmath
    inst, at = tr
    bad = []
    NL = 1 << depth
    for seg, vals in enumerate(inst):
        if vals is None:
            continue
        lo, up = float(got["gap"][seg][0]), float(got["gap"][seg][1])
        n_inst = len(vals) - 1
        leaf_lower = got.get("leaf_lower", [None] * len(inst))[seg]
        for j, v in enumerate(vals):
            if not mpmath.mpf(lo) <= v:
                bad.append(f"{tag} segment {seg}: lower {lo!r} above the truth {mpmath.nstr(v, 20)} at instant {j}/{n_inst}")
                break
            if leaf_lower is not None:
                l = min(j * NL // n_inst, NL - 1)
                ls = {l} | ({l - 1} if (j * NL) % n_inst == 0 and l > 0 and j < n_inst else set())
                if any(not mpmath.mpf(float(leaf_lower[x])) <= v for x in ls):
                    bad.append(f"{tag} segment {seg} leaf {l}: its L above the truth {mpmath.nstr(v, 20)} at instant {j}/{n_inst}")
                    break
        _, _, pu, wi = (int(x) for x in got["where"][seg])
        if pu < 0:      # (every witness of the segment was open: no upper bound)
            if up != np.inf:
                bad.append(f"{tag} segment {seg}: upper {up!r} without a witness")
        elif not at(seg, pu, wi, NL) <= mpmath.mpf(up):
            bad.append(f"{tag} segment {seg}: upper {up!r} below the truth at its witness ({pu}, {wi})")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
KINDS = ("alongside", "line", "five", "late", "early", "formation")


def _shift(track, off):
    T, C, s = track
    C = np.array(C, dtype=np.float64)
    C[:, :, 0] += np.asarray(off)[:, None]
    return T, C, s


def _side(rng, lo, hi):
    d = rng.uniform(-1.0, 1.0, size=3) * (1.0, 1.0, 0.3)
    return d / np.linalg.norm(d) * rng.uniform(lo, hi)


def obstacles_for(b, solve, seed, set_sizes, none_at=None, close=(0,), one_set=False, n_sets=None, with_start=True, with_radius=True,
                  uniform_one=False):
    """Obstacle sets for the batch b (moving_penalty_reference.batch): trajectory t avoids a set of set_sizes[t % len] tracks, whose kinds
    cycle through KINDS: alongside (the trajectory's own waypoints moved sideways by 1.3 .. 2 m, 0.05 s late: its knots straddle the
    leaves), line (ONE segment at constant velocity, higher coefficients zero: it waits, is met under way, has arrived), five (five
    segments), late (departs after the trajectory has landed: it waits for the whole flight), early (has arrived before the departure),
    formation (the trajectory's own track 1.5 m aside with the same departure).  Tracks pass 0.9 .. 2 m aside, those of the trajectories in
    `close` 0.15 .. 0.4 m.  Radii alternate 0 and 0.3.  one_set: ONE set (that of the longest trajectory) with NULL set_offsets / traj_set;
    n_sets = k: k sets, laid along the first k trajectories, and trajectory t avoids set t mod k;
    uniform_one: line tracks only (every obstacle track has ONE segment).  with_start / with_radius False: those arrays are NULL (zeros):
    the trajectories then all depart at 0."""
    rng = np.random.default_rng(seed)
    n = b["seg_offsets"].size - 1
    r = b["r"]
    traj_start = rng.uniform(-0.4, 0.6, size=n) if with_start else np.zeros(n)
    tracks, set_off = [], [0]
    todo = [int(np.argmax(np.diff(b["seg_offsets"])))] if one_set else range(n if n_sets is None else n_sets)
    for t in todo:
        size = set_sizes[t % len(set_sizes)]
        s0, s1 = int(b["seg_offsets"][t]), int(b["seg_offsets"][t + 1])
        F = float(np.sum(b["times"][s0:s1]))
        for j in range(size):
            kind = "line" if uniform_one else KINDS[j % len(KINDS)]
            near = t in close and j == 0
            off = _side(rng, 0.15, 0.4) if near else _side(rng, 0.9, 2.0)
            if kind == "alongside":
                tr = MP._track_alongside(b, t, solve, _side(rng, 0.15, 0.4) if near else _side(rng, 1.3, 2.0), traj_start[t])
            elif kind == "line":
                tr = _shift(MP._track_line(b, t, rng, traj_start[t]), off)
            elif kind == "five":
                tr = _shift(MP._track_five(b, t, solve, rng, traj_start[t]), off)
            elif kind == "late":
                T, C, _ = _shift(MP._track_line(b, t, rng, traj_start[t]), off)
                tr = (T, C, traj_start[t] + F + 0.3)
            elif kind == "early":
                T, C, _ = _shift(MP._track_line(b, t, rng, traj_start[t]), off)
                tr = (T, C, traj_start[t] - float(np.sum(T)) - 0.2)
            else:
                T, C, _ = MP._track_alongside(b, t, solve, (1.5, 0.0, 0.0), traj_start[t])
                tr = (T, C, traj_start[t])
            tracks.append(tr)
        set_off.append(len(tracks))
    obs = MP._pack(r, tracks)
    if uniform_one:
        obs["seg_offsets"] = None
        obs["uniform_segments"] = 1
    if not with_start:
        obs["start"] = None
    if with_radius:
        obs["radius"] = np.where(np.arange(len(tracks)) % 2 == 0, 0.0, 0.3)
    if one_set:
        return obs
    traj_set = (np.arange(n) % (n if n_sets is None else n_sets)).astype(np.int32)
    if none_at is not None:
        traj_set[none_at] = -1
    obs.update(set_offsets=np.array(set_off, dtype=np.int32), traj_set=traj_set)
    if with_start:
        obs["traj_start"] = traj_start
    return obs


def line_track(r, p0, vel, T):
    """ONE segment of duration T at constant velocity from p0: coefficients [3][1][2r]"""
    c = np.zeros((3, 1, 2 * r))
    c[:, 0, 0] = p0
    c[:, 0, 1] = vel
    return c


def single_case(r, T, C, tracks, traj_start=0.0):
    """one trajectory (T [M], C [3][M][2r]) against tracks = [(T_o, C_o, start_o, radius_o)] in the C-ABI layout: (so, times, coeff, obstacles)"""
    so = np.array([0, len(T)], dtype=np.int32)
    obs = MP._pack(r, [(np.asarray(To, dtype=np.float64), Co, st) for (To, Co, st, _) in tracks])
    obs["radius"] = np.array([t[3] for t in tracks], dtype=np.float64)
    obs["traj_start"] = np.array([traj_start], dtype=np.float64)
    return so, np.asarray(T, dtype=np.float64), np.asarray(C, dtype=np.float64).ravel(), obs


ROUNDED_ENDS = ((0.1, 0.7), (0.3, 0.6), (0.7, 0.1), (0.2, 0.9), (1.1, 0.3), (0.1, 0.2), (2.3, 0.4), (0.6, 0.3))


def rounded_end_case(r, S, T0, near_after):
    """ONE segment from S to S + T0 along x at 1 m/s against an obstacle that stands 2 m (0.3 m) beside the path and jumps to 0.3 m (2 m)
    beside it at a knot that is the DOUBLE fl(S + T0): -> (so, times, coeff, obstacles, the knot, the real arrival as a Fraction)"""
    K1 = float(np.float64(S) + np.float64(T0))
    y = (2.0, 0.3) if near_after else (0.3, 2.0)
    Co = np.zeros((3, 2, 2 * r))
    Co[:, 0, 0], Co[:, 1, 0] = (0.5, y[0], 1.0), (0.5, y[1], 1.0)
    case = single_case(r, [T0], line_track(r, (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), T0), [(np.array([K1, 0.6]), Co, 0.0, 0.0)], traj_start=S)
    return case + (K1, Fraction(S) + Fraction(T0))


def formation_case(r, solve):
    """a track that is the trajectory's own, 1.5 m aside, with the same departure, dyadic durations and radius 0.25"""
    rng = np.random.default_rng(5)
    T = np.array([0.5, 0.25, 1.0, 0.5])
    w = np.cumsum(rng.uniform(-1.0, 1.0, size=(5, 3)), axis=0)
    Ct = solve(r, w, np.zeros((2, r - 1, 3)), T)
    Co = Ct.copy()
    Co[0, :, 0] += 1.5
    return single_case(r, T, Ct, [(T, Co, 0.25, 0.25)], traj_start=0.25)


def head_on(r):
    """What the feature is for: a head-on pass on straight lines, 10 m/s closing speed, lateral offset 0.2 m, ONE segment of 1 s.  The
    vehicle flies +x at 5 m/s from x = -2.5, the obstacle -x at 5 m/s from x = +2.5 + 0.3125, so that the closest approach (0.2 m) falls
    in the middle between two of the eight samples."""
    C = line_track(r, (-2.5, 0.0, 1.0), (5.0, 0.0, 0.0), 1.0)
    Co = line_track(r, (2.5 + 0.625, 0.2, 1.0), (-5.0, 0.0, 0.0), 1.0)
    return single_case(r, [1.0], C, [([1.0], Co, 0.0, 0.0)])


# the batches of the GPU parity test (the CPU test qualifies them): ragged M in 1..11 -- a one-segment trajectory, and 9, 10, 11: a second
# round of eight segments
RAGGED = (9, 1, 5, 10, 2, 6, 11, 3, 7)
GPU_D_REQ = 0.8


def gpu_cases():
    ragged = list(RAGGED)
    return {
        "lone_uniform_M8_r4": dict(r=4, Ms=(8,), uniform=True, seed=5, set_sizes=(2,), opts=dict()),
        "n7_ragged_r3": dict(r=3, Ms=tuple(ragged[:7]), uniform=False, seed=6, set_sizes=(1, 2, 0), opts=dict(none_at=3, n_sets=3)),
        "n9_ragged_r4_nine": dict(r=4, Ms=tuple(ragged), uniform=False, seed=7, set_sizes=(1, 9, 2), opts=dict()),
        "n67_uniform_M8_r3_one_set": dict(r=3, Ms=(8,) * 67, uniform=True, seed=8, set_sizes=(2,),
                                          opts=dict(one_set=True, with_start=False, with_radius=False, uniform_one=True), shared=True),
    }


GPU_DEPTHS = (0, 2, 3, 5)


@functools.lru_cache(maxsize=None)
def _batch(r, Ms, seed, shared):
    return MP.batch(r, Ms, seed, shared=shared)


def gpu_batch(name):
    c = gpu_cases()[name]
    return _batch(c["r"], c["Ms"], c["seed"], bool(c.get("shared", False)))


def gpu_obstacles(name, solve):
    c = gpu_cases()[name]
    return obstacles_for(gpu_batch(name), solve, c["seed"] + 100, c["set_sizes"], **c["opts"])


def covering_lines(b, seed, per_set=2):
    """For the cross-check against the penalty: per trajectory a set of `per_set` ONE-segment constant-velocity tracks that pass 0.6 .. 1.5 m
    from its middle waypoint, depart 1 s before it and arrive 1 s after it has landed -- no sample of the penalty falls near an obstacle
    knot, so the penalty's sampling rule (with its 1e-4 s of overhang) and the certified curve are the same positions."""
    rng = np.random.default_rng(seed)
    so, r = b["seg_offsets"], b["r"]
    n = so.size - 1
    traj_start = rng.uniform(-0.4, 0.6, size=n)
    tracks, set_off = [], [0]
    for t in range(n):
        s0, s1 = int(so[t]), int(so[t + 1])
        F = float(np.sum(b["times"][s0:s1]))
        mid = b["waypoints"][s0 + t + (s1 - s0) // 2]
        for _ in range(per_set):
            vel = rng.uniform(-1.0, 1.0, size=3) * (1.0, 1.0, 0.2)
            Do = F + 2.0
            p0 = mid + _side(rng, 0.6, 1.5) - vel * (1.0 + 0.5 * F)
            tracks.append((np.array([Do]), line_track(r, p0, vel, Do), traj_start[t] - 1.0))
        set_off.append(len(tracks))
    obs = MP._pack(r, tracks)
    obs.update(radius=rng.uniform(0.0, 0.3, size=len(tracks)), set_offsets=np.array(set_off, dtype=np.int32),
               traj_set=np.arange(n, dtype=np.int32), traj_start=traj_start)
    return obs
