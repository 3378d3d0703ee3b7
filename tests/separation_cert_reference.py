"""CPU reference of uavqp_separation_certificate_* (include/uavqp.h): the method of csrc/qp_separation_cert.h restated in numpy float64 with
the kernel's order of operations (certificate), an independent TRUTH (truth: the definition of the certified curve evaluated with mpmath at
60 digits), and the inputs the CPU test (tests/test_separation_cert_reference.py) qualifies for the GPU test
(tests/test_gpu_separation_cert.py).

The certified curve.  The clock knots of vehicle b are the DOUBLES K_0 = start_b, K_{m+1} = fl(K_m + T_m).  q_b(t) is segment 0 at local time
0 for t <= K_0, segment m at local time t - K_m (real arithmetic) for t in [K_m, K_{m+1}], the last segment at T_{M-1} for t >= K_M; pieces
are closed (at a knot both values belong to the curve).  s_ij(t) = sqrt(dx^2 + dy^2 + (dz / downwash)^2) of q_i(t) - q_j(t).
Leaves: tau_w = the double nearest to clock_start + w dt / 2^depth, w = 0..NL, NL = n_cells 2^depth; leaf l = [tau_l, tau_{l+1}].

The method, n = 2r - 1.  Per (vehicle, leaf) every segment whose closed piece meets the leaf is restricted to it: envelope_reference.bernstein
on the segment, a de Casteljau split at lambda_1 = lb / T_m keeping the left half, one at lambda_2 = la / lb keeping the right half, with
la = max(tau_l - K_m, 0), lb = min(tau_{l+1} - K_m, T_m), both ratios clamped to [0, 1] (NaN counts as 0); waiting is segment 0 at
lambda_1 = lambda_2 = 0, arrived (tau_l >= K_M) the last segment at lambda_1 = lambda_2 = 1.  A leaf inside ONE piece is a SINGLE entry (its
3 x (n + 1) coefficients), any other a BOX entry (per-axis [lo, hi] over the coefficients of its pieces, the left end = coefficient 0 of the
first piece, the right end = coefficient n of the last).  Guard per axis: the largest over the pieces of
    G_x = (64 (n + 1) + 2 n kappa) 2^-53 S_x,   S_x = sum_k |c_k T^k|,   kappa = max(|K_m|, |K_{m+1}|) / T_m
(in units of 2^-53 S: the Bernstein conversion 16 (n + 1), two splits of n levels with a rounded weight 6 n, four roundings of the ratios
times |dp/du| <= n S gives 8 n, together under 30 (n + 1); 2 n kappa covers the part of the piece beyond u = 1 that the ROUNDED knot
K_{m+1} admits).  Pair (i, j) on a leaf, Gs = G_i + G_j: both single, [lo_x, hi_x] = [min_k, max_k] of b_ik - b_jk; otherwise the interval
difference of the boxes; lo -= Gs, hi += Gs, g_x = max(0, lo_x, -hi_x),
    L = sqrt(g_x^2 + g_y^2 + (g_z / downwash)^2) - R,                R = 16 2^-53 sum_x max(|lo_x|, |hi_x|)
    U = s(d) + sqrt(3) max_x Gs_x + 16 2^-53 (|d_x| + |d_y| + |d_z|)   d = the difference of the two entries' end positions
lower_i = max(0, min L), upper_i = min U; ties: the smaller partner, then the smaller index.
ALLOWANCE of a pair on a leaf: sqrt(3) max_x Gs_x + R, within which two evaluations of these formulas agree."""
import bisect
import functools
from fractions import Fraction

import numpy as np

import envelope_reference as E
import swarm_reference as SW

EPS = 2.0 ** -53
SQRT3 = 1.7320508075688772
CERTIFIED, VIOLATED, MOVING = 1, 2, 4
SOLVED = 1
MAX_VEHICLES = 128
SINGLE, BOX = 0, 1
DEFAULTS = dict(depth=2, n_cells=64, clock_start=0.0, dt=0.1, downwash=1.0, d_req=1.0)
OUT = ("lower", "upper", "where", "verdict", "group_verdict")


def taus(depth, n_cells, clock_start, dt):
    """tau_w, w = 0..NL: the double nearest to clock_start + w (dt / 2^depth)"""
    h = Fraction(float(dt)) / (1 << depth)
    return np.array([float(Fraction(float(clock_start)) + w * h) for w in range((n_cells << depth) + 1)])


def knots(T, start):
    K = [float(start)]
    for t in T:
        K.append(K[-1] + float(t))
    return K


def restrict(b, lam1, lam2):
    """b [n][nc] Bernstein on [0, 1] -> on [lam2 lam1, lam1]: the left half of a split at lam1, then the right half of one at lam2"""
    w = b.copy()
    n1 = w.shape[1] - 1
    l1, o1 = lam1[:, None], (1.0 - lam1)[:, None]
    for k in range(1, n1 + 1):
        w[:, k:] = l1 * w[:, k:] + o1 * w[:, k - 1:n1]
    l2, o2 = lam2[:, None], (1.0 - lam2)[:, None]
    for k in range(1, n1 + 1):
        w[:, :n1 - k + 1] = l2 * w[:, 1:n1 - k + 2] + o2 * w[:, :n1 - k + 1]
    return w


def ratio(x):
    return np.fmin(np.fmax(x, 0.0), 1.0)      # (fmax / fmin drop a NaN: 0 / 0 counts as 0)


def entries(T, C, start, tw, force_box=False):
    """The entries of one vehicle (durations T [M], coefficients C [3][M][nc]) on the leaves of tw: dict of arrays over the leaves."""
    M, nc = len(T), C.shape[2]
    ta, tb = tw[:-1], tw[1:]
    NL = ta.size
    K = knots(T, start)
    e = dict(kind=np.full(NL, BOX), coef=np.zeros((NL, 3, nc)), lo=np.zeros((NL, 3)), hi=np.zeros((NL, 3)), G=np.zeros((NL, 3)),
             left=np.zeros((NL, 3)), right=np.zeros((NL, 3)), K=K, state=np.zeros(NL, dtype=int))
    pieces = np.zeros(NL, dtype=int)

    def add(mask, m, lam1, lam2):
        if not mask.any():
            return
        with np.errstate(all="ignore"):
            kappa = max(abs(K[m]), abs(K[m + 1])) / np.float64(T[m])
            b, S = E.bernstein(C[:, m, :], np.full(3, T[m]), 0)
            g = (64.0 * nc + 2.0 * (nc - 1) * kappa) * EPS * S
            first = pieces[mask] == 0
            for ax in range(3):
                w = restrict(np.repeat(b[ax][None, :], int(mask.sum()), axis=0), lam1, lam2)
                l, u = w.min(axis=1), w.max(axis=1)
                e["lo"][mask, ax] = np.where(first, l, np.fmin(e["lo"][mask, ax], l))
                e["hi"][mask, ax] = np.where(first, u, np.fmax(e["hi"][mask, ax], u))
                G = e["G"][mask, ax]
                e["G"][mask, ax] = np.where(first | (g[ax] > G) | np.isnan(g[ax]), g[ax], G)
                e["left"][mask, ax] = np.where(first, w[:, 0], e["left"][mask, ax])
                e["right"][mask, ax] = w[:, -1]
                e["coef"][mask, ax] = w
        pieces[mask] += 1

    waiting = tb <= K[0]
    n = int(waiting.sum())
    add(waiting, 0, np.zeros(n), np.zeros(n))
    done = waiting.copy()
    for m in range(M):
        touch = ~done & (K[m] <= tb) & ((K[m + 1] > ta) | ((K[m + 1] == ta) & (m < M - 1)))      # (K_M = tau_l: arrived)
        inside = touch & (K[m] <= ta) & (tb <= K[m + 1])
        pieces[inside] = 0
        with np.errstate(all="ignore"):
            la, lb = np.fmax(ta[touch] - K[m], 0.0), np.fmin(tb[touch] - K[m], T[m])
            add(touch, m, ratio(lb / np.float64(T[m])), ratio(la / lb))
        done |= inside
    arrived = pieces == 0
    n = int(arrived.sum())
    add(arrived, M - 1, np.ones(n), np.ones(n))
    single = waiting | (done & ~waiting) | arrived
    e["kind"] = np.where(single & (not force_box), SINGLE, BOX)
    e["state"] = np.where(waiting, 1, np.where(arrived, 2, np.where(single, 0, 3)))      # moving / waiting / arrived / straddling
    return e


def _norm(d, inv_dw):
    z = d[..., 2] * inv_dw
    return np.sqrt(d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + z * z))


def pair(ei, ej, inv_dw):
    """(L [NL], U [NL + 1], allowance of L [NL], allowance of U [NL + 1], bad) of the pair; the numbers of (j, i) are the same"""
    with np.errstate(all="ignore"):
        Gs = ei["G"] + ej["G"]
        Gmax = np.max(Gs, axis=1)
        bad = bool(np.any(~(Gmax < np.inf)))
        both = (ei["kind"] == SINGLE) & (ej["kind"] == SINGLE)
        d = ei["coef"] - ej["coef"]
        lo = np.where(both[:, None], d.min(axis=2), ei["lo"] - ej["hi"]) - Gs
        hi = np.where(both[:, None], d.max(axis=2), ei["hi"] - ej["lo"]) + Gs
        g = np.fmax(0.0, np.fmax(lo, -hi))
        R = 16.0 * EPS * np.sum(np.fmax(np.abs(lo), np.abs(hi)), axis=1)
        L = _norm(g, inv_dw) - R
        pad = SQRT3 * Gmax
        dl, dr = ei["left"] - ej["left"], ei["right"][-1] - ej["right"][-1]
        Rl, Rr = 16.0 * EPS * np.sum(np.abs(dl), axis=1), 16.0 * EPS * np.sum(np.abs(dr))
        U = np.concatenate([_norm(dl, inv_dw) + pad + Rl, [_norm(dr, inv_dw) + pad[-1] + Rr]])
        aU = np.concatenate([pad + Rl, [pad[-1] + Rr]])
    return L, U, pad + R, aU, bad


def _pick(vals):
    """vals: list of (partner, array) in rising partner order -> (value, partner, index, runner-up - value) with the kernel's tie rule"""
    best = (np.inf, -1, 0)
    for p, a in vals:
        k = int(np.argmin(a))
        if a[k] < best[0]:
            best = (float(a[k]), p, k)
    if best[1] < 0:
        return np.inf, -1, 0, np.inf
    rest = np.concatenate([np.delete(a, best[2]) if p == best[1] else a for p, a in vals])
    return best + (float(rest.min() - best[0]) if rest.size else np.inf,)


def certificate(r, seg_offsets, times, coeff, group_offsets=None, start=None, status=None, force_box=False, **params):
    """The method of qp_separation_cert.h.  Returns the five outputs of uavqp_separation_certificate_* and, for the tests, per vehicle:
    allow_lower / allow_upper (the allowance of the winning pair), gap_lower / gap_upper (how far the runner-up candidate is from the winner),
    and over the batch: states (which of moving / waiting / arrived / straddling leaves occurred) and knot_margin (the smallest distance of
    a knot K_m from a leaf end)."""
    p = dict(DEFAULTS, **params)
    so = np.asarray(seg_offsets, dtype=np.int64)
    n_traj, nc = so.size - 1, 2 * r
    go = np.array([0, n_traj]) if group_offsets is None else np.asarray(group_offsets, dtype=np.int64)
    start = np.zeros(n_traj) if start is None else np.asarray(start, dtype=np.float64)
    times = np.asarray(times, dtype=np.float64)
    coeff = np.asarray(coeff, dtype=np.float64)
    tw = taus(p["depth"], p["n_cells"], p["clock_start"], p["dt"])
    inv_dw = 1.0 / float(p["downwash"])
    out = dict(lower=np.full(n_traj, np.inf), upper=np.full(n_traj, np.inf), where=np.tile(np.array([-1, 0, -1, 0], dtype=np.int32), (n_traj, 1)),
               verdict=np.zeros(n_traj, dtype=np.int32), group_verdict=np.zeros(go.size - 1, dtype=np.int32),
               allow_lower=np.zeros(n_traj), allow_upper=np.zeros(n_traj), gap_lower=np.full(n_traj, np.inf), gap_upper=np.full(n_traj, np.inf),
               states=set(), knot_margin=np.inf)
    for g in range(go.size - 1):
        bs = list(range(int(go[g]), int(go[g + 1])))
        if len(bs) > MAX_VEHICLES:
            out["lower"][bs] = out["upper"][bs] = np.nan
            continue
        live = [b for b in bs if so[b + 1] > so[b] and (status is None or int(status[b]) == SOLVED)]
        ent = {}
        for b in live:
            T, C = SW.split(r, so, times, coeff, b)
            ent[b] = entries(T, C, start[b], tw, force_box)
            out["states"] |= set(ent[b]["state"].tolist())
            K = np.array(ent[b]["K"])
            out["knot_margin"] = min(out["knot_margin"], float(np.min(np.abs(K[:, None] - tw[None, :]))))
        pairs, bad = {}, set()
        for x, i in enumerate(live):
            for j in live[x + 1:]:
                pairs[i, j] = pairs[j, i] = q = pair(ent[i], ent[j], inv_dw)
                if q[4]:
                    bad |= {i, j}
        cert, other = CERTIFIED, 0
        for i in live:
            word = 0
            if i in bad:
                out["lower"][i] = out["upper"][i] = np.nan
            else:
                others = [j for j in live if j != i]
                Lv, Lp, Ll, out["gap_lower"][i] = _pick([(j, pairs[i, j][0]) for j in others])
                Uv, Up, Uw, out["gap_upper"][i] = _pick([(j, pairs[i, j][1]) for j in others])
                if Lp >= 0:
                    out["lower"][i], out["upper"][i] = max(0.0, Lv), Uv
                    out["where"][i] = [Lp, Ll, Up, Uw]
                    out["allow_lower"][i], out["allow_upper"][i] = pairs[i, Lp][2][Ll], pairs[i, Up][3][Uw]
                moving = ent[i]["K"][-1] > tw[-1]
                word = (CERTIFIED if out["lower"][i] >= p["d_req"] else 0) | (VIOLATED if out["upper"][i] < p["d_req"] else 0) | (MOVING if moving else 0)
            out["verdict"][i] = word
            cert &= word
            other |= word
        out["group_verdict"][g] = (cert | (other & (VIOLATED | MOVING))) if live else 0
    return out


def state(word):
    return "certified" if word & CERTIFIED else "violated" if word & VIOLATED else "undecided"


def two_allowances_away(ref, d_req):
    """d_req lies more than two allowances from every finite bound: no verdict bit hangs on a rounding"""
    lo, up = ref["lower"], ref["upper"]
    ok_lo = ~np.isfinite(lo) | (np.abs(lo - d_req) > 2.0 * ref["allow_lower"])
    ok_up = ~np.isfinite(up) | (np.abs(up - d_req) > 2.0 * ref["allow_upper"])
    return bool(np.all(ok_lo & ok_up))


def where_comparable(ref):
    """per vehicle: the runner-up candidate of lower (of upper) is more than two allowances from the winner, so that `where` is no tie"""
    return ref["gap_lower"] > 2.0 * ref["allow_lower"], ref["gap_upper"] > 2.0 * ref["allow_upper"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the truth (mpmath, 60 digits): the definition, nothing of the method
# ---------------------------------------------------------------------------------------------------------------------------------------
def _positions(mp, T, C, K, t):
    """every value of the curve of one vehicle at the instant t (mpf): one, or two at a knot"""
    M = len(T)
    Km = [mp.mpf(k) for k in K]

    def at(m, tl):
        out = []
        for ax in range(3):
            v = mp.mpf(0)
            for c in C[ax][m][::-1]:
                v = v * tl + mp.mpf(float(c))
            out.append(v)
        return out

    vals = []
    if t <= Km[0]:
        vals.append(at(0, mp.mpf(0)))
    m0 = bisect.bisect_right(K, float(t)) - 1
    for m in range(max(m0 - 1, 0), min(m0 + 2, M)):
        if Km[m] <= t <= Km[m + 1]:
            vals.append(at(m, t - Km[m]))
    if t >= Km[M]:
        vals.append(at(M - 1, mp.mpf(float(T[M - 1]))))
    return vals


def truth(r, seg_offsets, times, coeff, group_offsets=None, start=None, status=None, per_leaf=64, truth_depth=3, extra=(), **params):
    """min over the instants and the partners of s_ij(t), per vehicle, on per_leaf instants of every leaf of depth truth_depth (the left
    end included, and the window's last instant) -> (min_sep [n_traj] of mpf (None: no partner), at(i, j, t) the truth at any instant)."""
    import mpmath
    mp = mpmath.mp
    mp.dps = 60
    p = dict(DEFAULTS, **params)
    so = np.asarray(seg_offsets, dtype=np.int64)
    n_traj = so.size - 1
    go = np.array([0, n_traj]) if group_offsets is None else np.asarray(group_offsets, dtype=np.int64)
    start = np.zeros(n_traj) if start is None else np.asarray(start, dtype=np.float64)
    tw = taus(truth_depth, p["n_cells"], p["clock_start"], p["dt"])
    inst = []
    for l in range(tw.size - 1):
        a, b = mp.mpf(float(tw[l])), mp.mpf(float(tw[l + 1]))
        inst += [a + (b - a) * k / per_leaf for k in range(per_leaf)]
    inst.append(mp.mpf(float(tw[-1])))
    inst += [mp.mpf(float(t)) for t in extra]
    dw = mp.mpf(float(p["downwash"]))
    veh = {}
    for b in range(n_traj):
        if so[b + 1] > so[b] and (status is None or int(status[b]) == SOLVED):
            T, C = SW.split(r, so, np.asarray(times, dtype=np.float64), np.asarray(coeff, dtype=np.float64), b)
            veh[b] = (T, C, knots(T, start[b]))

    def sep(P, Q):
        return min(mp.sqrt((a[0] - c[0]) ** 2 + (a[1] - c[1]) ** 2 + ((a[2] - c[2]) / dw) ** 2) for a in P for c in Q)

    def at(i, j, t):
        t = mp.mpf(float(t))
        return sep(_positions(mp, *veh[i], t), _positions(mp, *veh[j], t))

    best = [None] * n_traj
    for g in range(go.size - 1):
        live = [b for b in range(int(go[g]), int(go[g + 1])) if b in veh]
        if len(live) < 2:
            continue
        for t in inst:
            P = {b: _positions(mp, *veh[b], t) for b in live}
            for x, i in enumerate(live):
                for j in live[x + 1:]:
                    s = sep(P[i], P[j])
                    for b in (i, j):
                        if best[b] is None or s < best[b]:
                            best[b] = s
    return best, at


def soundness_failures(got, tr, tw, tag=""):
    """lower <= truth at every instant and truth(witness) <= upper, in mpmath arithmetic and WITHOUT a tolerance -> list of strings.
    got: lower, upper, where of the method (reference or device); tr: truth(); tw: the tau_w of got's depth."""
    import mpmath
    best, at = tr
    bad = []
    for i, m in enumerate(best):
        lo, up = float(got["lower"][i]), float(got["upper"][i])
        if m is None:
            if not (lo == np.inf and up == np.inf):
                bad.append(f"{tag} vehicle {i}: no partner, but bounds {lo}, {up}")
            continue
        if not mpmath.mpf(lo) <= m:
            bad.append(f"{tag} vehicle {i}: lower {lo!r} above the truth {mpmath.nstr(m, 20)}")
        _, _, pu, w = (int(x) for x in got["where"][i])
        if pu < 0 or not at(i, pu, tw[w]) <= mpmath.mpf(up):
            bad.append(f"{tag} vehicle {i}: upper {up!r} below the truth at its witness ({pu}, {w})")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def solve(oracle, b):
    """the coefficients of a batch (make_batch) by the CPU oracle's exact solve, in the layout of the device ([3][M][2r] per trajectory)"""
    r, so, out = b["r"], b["so"], []
    for t in range(so.size - 1):
        s0, s1 = int(so[t]), int(so[t + 1])
        wp, T, bc = b["wp"][s0 + t:s1 + t + 1], b["T"][s0:s1], b["bc"][t]
        out.extend(np.asarray(oracle.solve_exact(r, wp[:, ax], bc[0, :, ax], bc[1, :, ax], T), dtype=np.float64).ravel() for ax in range(3))
    return np.concatenate(out)


def make_batch(r, sizes, Ms, seed, spread=None, **scene):
    """A batch of swarms in the C-ABI layout: swarm g flies through a region 10 g m along x (swarm_reference.scene); the swarm `spread` is
    laid out 5 m apart."""
    rng = np.random.default_rng(seed)
    wps, Ts, starts, b = [], [], [], 0
    for g, A in enumerate(sizes):
        w, T, s = SW.scene(rng, Ms[b:b + A], centre=(10.0 * g, 0.0, 1.0), spread=5.0 if g == spread else 0.0, **scene)
        wps += w
        Ts += T
        starts.append(s)
        b += A
    n = sum(sizes)
    bc = rng.uniform(-0.3, 0.3, size=(n, 2, r - 1, 3))
    return dict(r=r, so=np.concatenate([[0], np.cumsum(Ms)]).astype(np.int32), wp=np.concatenate(wps), T=np.concatenate(Ts), bc=bc,
                go=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), start=np.concatenate(starts))


# the small swarms the CPU test checks against the truth (and the GPU test checks the device's own numbers against)
SMALL_SIZES = (2, 3, 5, 1)
SMALL_CLOCK = dict(n_cells=8, clock_start=-0.2, dt=0.4, d_req=0.6)


@functools.lru_cache(maxsize=None)
def small_batch(r, downwash):
    n = sum(SMALL_SIZES)
    Ms = [1 + (4 * b + 3) % 11 for b in range(n)]
    Ms[2] = 1
    return make_batch(r, SMALL_SIZES, Ms, seed=11 + r, start_span=(-0.1, 1.1)), dict(SMALL_CLOCK, downwash=downwash)


# the batches of the GPU parity test: 95 vehicles in swarms of 2, 70, 1, 9, 4, 3 and 6 (the swarm of 4 spread 5 m apart), and one swarm of
# exactly 128 vehicles with M = 2 (a tile is 2 leaves)
GPU_SIZES = (2, 70, 1, 9, 4, 3, 6)
GPU_SPREAD = 4
GPU_KINDS = {"uniform_M8_r4": (4, True), "ragged_M1to11_r3": (3, False), "ragged_M1to11_r4": (4, False)}
GPU_CLOCKS = ((0, 40), (2, 7), (4, 1), (4, 7))      # (depth, n_cells): depth 0, 2, 4 and 1, 7, 40 cells


def gpu_clock(depth, n_cells):
    """the window runs from -0.1 s to 2.6 s (n_cells = 1: one cell from 0.9 s, most vehicles in flight)"""
    t0 = 0.9 if n_cells == 1 else -0.1
    return dict(depth=depth, n_cells=n_cells, clock_start=t0, dt=(2.6 - t0) / n_cells if n_cells > 1 else 0.37, downwash=1.5, d_req=0.1)


@functools.lru_cache(maxsize=None)
def gpu_batch(kind):
    r, uniform = GPU_KINDS[kind]
    n = sum(GPU_SIZES)
    Ms = [8] * n if uniform else [1 + (4 * b) % 11 for b in range(n)]
    return make_batch(r, GPU_SIZES, Ms, seed=3, spread=GPU_SPREAD, start_span=(-0.3, 1.0))


@functools.lru_cache(maxsize=None)
def full_swarm_batch(r):
    return make_batch(r, (128,), [2] * 128, seed=5, radius=6.0, start_span=(-0.3, 0.6))


FULL_CLOCK = dict(depth=2, n_cells=3, clock_start=-0.1, dt=0.9, downwash=1.0, d_req=0.3)
