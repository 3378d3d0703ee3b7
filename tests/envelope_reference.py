"""CPU reference of uavqp_envelope_* (include/uavqp.h): the method of qp_envelope.h restated in numpy float64 (envelope), and the exact
extrema of the same quantities by mpmath at 60 digits (exact_extrema): roots of the derivative of the polynomial, or of the squared-norm
polynomial, plus the two ends.  The recorded cases (cases, needs the CPU oracle) are written to tests/golden/envelope_exact.json by
tests/golden/gen_envelope_exact.py; the tests read that file (load_golden)."""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "envelope_exact.json")
GRAVITY = 9.81
EPS = 2.0 ** -53
TESTS = ("v_max", "a_max", "j_max", "f_min", "f_max", "tilt_max", "box")
NORMS = ("|v|", "|a|", "|j|", "thrust", "w")
TILT_GOLDEN = 0.6   # tilt_max of the recorded w
SOLVED = 1          # UAVQP_SOLVED


def falling(k, d):
    f = 1.0
    for j in range(d):
        f *= float(k - j)
    return f


def segment_coefficients(r, seg_offsets, coeff):
    """[sum M][3][2r] from the library's layout: per trajectory [axis][segment][2r]"""
    nc = 2 * r
    so = np.asarray(seg_offsets, dtype=np.int64)
    coeff = np.asarray(coeff, dtype=np.float64).ravel()
    out = np.zeros((int(so[-1]), 3, nc))
    for b in range(so.size - 1):
        s0, M = int(so[b]), int(so[b + 1] - so[b])
        if M > 0:
            out[s0:s0 + M] = coeff[3 * nc * s0:3 * nc * (s0 + M)].reshape(3, M, nc).transpose(1, 0, 2)
    return out


def bernstein(C, T, D):
    """C [n][2r] monomials in t, T [n]: (b [n][m+1] Bernstein coefficients of the D-th derivative on u = t / T, S [n])"""
    nc = C.shape[-1]
    m = nc - 1 - D
    a = np.stack([falling(k + D, D) * C[:, k + D] * T ** k for k in range(m + 1)], axis=-1)
    S = np.sum(np.abs(a), axis=-1)
    b = np.zeros_like(a)
    for i in range(m + 1):
        for k in range(i + 1):
            b[:, i] += (math.comb(i, k) / math.comb(m, k)) * a[:, k]
    return b, S


def split(w):
    """one level of midpoint de Casteljau on [..., m+1]: (left half, right half)"""
    m = w.shape[-1] - 1
    left, right = np.empty_like(w), np.empty_like(w)
    cur = w
    left[..., 0], right[..., m] = cur[..., 0], cur[..., m]
    for k in range(1, m + 1):
        cur = 0.5 * (cur[..., :-1] + cur[..., 1:])
        left[..., k], right[..., m - k] = cur[..., 0], cur[..., -1]
    return left, right


def scan(b, depth):
    """b [n][m+1]: (min, end min, end max, max) [n][4] over all 2^depth leaves; no guard"""
    leaves = b[:, None, :]
    for _ in range(depth):
        left, right = split(leaves)
        leaves = np.concatenate([left, right], axis=1)
    ends = leaves[:, :, [0, -1]]
    return np.stack([leaves.min(axis=(1, 2)), ends.min(axis=(1, 2)), ends.max(axis=(1, 2)), leaves.max(axis=(1, 2))], axis=-1)


def guarded(q, G):
    out = q.copy()
    out[:, 0] -= G
    out[:, 3] += G
    out[~(G < np.inf)] = np.nan
    return out


def square(bx, by, bz, zz_only=False):
    """Bernstein coefficients [n][2m+1] of the sum of squares of three polynomials given by theirs"""
    m = bx.shape[-1] - 1
    q = np.zeros(bx.shape[:-1] + (2 * m + 1,))
    for k in range(2 * m + 1):
        for i in range(max(0, k - m), min(m, k) + 1):
            wgt = math.comb(m, i) * math.comb(m, k - i) / math.comb(2 * m, k)
            d = bz[:, i] * bz[:, k - i]
            if not zz_only:
                d = bx[:, i] * bx[:, k - i] + by[:, i] * by[:, k - i] + d
            q[:, k] += wgt * d
    return q


def rooted(sq):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(sq), np.nan, np.sqrt(np.maximum(0.0, sq)))


def bits_upper(k, sq, G, lim2):
    if not lim2 > 0.0:
        return np.zeros(sq.shape[0], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        return ((sq[:, 3] <= lim2).astype(np.int64) | ((sq[:, 2] - G > lim2).astype(np.int64) << 1)) << (2 * k)


def bits_lower(k, sq, G, lim2):
    if not lim2 > 0.0:
        return np.zeros(sq.shape[0], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        return ((sq[:, 0] >= lim2).astype(np.int64) | ((sq[:, 1] + G < lim2).astype(np.int64) << 1)) << (2 * k)


def envelope(r, seg_offsets, times, coeff, status=None, depth=4, box_lo=None, box_hi=None, v_max=0.0, a_max=0.0, j_max=0.0, f_min=0.0,
             f_max=0.0, tilt_max=0.0):
    """The method of qp_envelope.h.  Returns the five outputs of uavqp_envelope_* (range, norm, peak, seg_verdict, verdict) and, for the
    tolerances of the tests: G [sum M][4][3] the guards of the ranges, Gq [sum M][5] the guards of the SQUARES (of w itself), sq [sum M][5][4]
    the guarded squares the verdict is taken on."""
    so = np.asarray(seg_offsets, dtype=np.int64)
    n_traj, tot = so.size - 1, int(so[-1])
    T = np.asarray(times, dtype=np.float64).ravel()
    C = segment_coefficients(r, so, coeff)
    rng, G = np.zeros((tot, 4, 3, 4)), np.zeros((tot, 4, 3))
    sq, Gq = np.zeros((tot, 5, 4)), np.zeros((tot, 5))
    bits = np.zeros(tot, dtype=np.int64)
    cos2 = math.cos(tilt_max) * math.cos(tilt_max)
    with np.errstate(all="ignore"):
        for D in range(4):
            m = 2 * r - 1 - D
            b, S = [], []
            for ax in range(3):
                bb, SS = bernstein(C[:, ax], T, D)
                b.append(bb)
                S.append(SS)
                G[:, D, ax] = 16.0 * float(m + 1) * EPS * SS
                rng[:, D, ax] = guarded(scan(bb, depth), G[:, D, ax])
            if D == 0:
                if box_lo is not None:
                    lo, hi = np.asarray(box_lo, dtype=np.float64).reshape(tot, 3), np.asarray(box_hi, dtype=np.float64).reshape(tot, 3)
                    cb = np.all((lo <= rng[:, 0, :, 0]) & (rng[:, 0, :, 3] <= hi), axis=1)
                    vb = np.any((rng[:, 0, :, 1] + G[:, 0] < lo) | (rng[:, 0, :, 2] - G[:, 0] > hi), axis=1)
                    bits |= (cb.astype(np.int64) | (vb.astype(np.int64) << 1)) << 12
                continue
            which = D - 1   # |v|, |a|, |j|
            Gq[:, which] = 32.0 * float(2 * m + 1) * EPS * (S[0] * S[0] + S[1] * S[1] + S[2] * S[2])
            sq[:, which] = guarded(scan(square(b[0], b[1], b[2]), depth), Gq[:, which])
            bits |= bits_upper(which, sq[:, which], Gq[:, which], [v_max * v_max, a_max * a_max, j_max * j_max][which])
            if D == 2:
                Sz = S[2] - np.abs(b[2][:, 0]) + np.abs(b[2][:, 0] + GRAVITY)
                bz = b[2] + GRAVITY
                qt, qz = square(b[0], b[1], bz), square(b[0], b[1], bz, zz_only=True)
                Gq[:, 3] = Gq[:, 4] = 32.0 * float(2 * m + 1) * EPS * (S[0] * S[0] + S[1] * S[1] + Sz * Sz)
                sq[:, 3] = guarded(scan(qt, depth), Gq[:, 3])
                bits |= bits_lower(3, sq[:, 3], Gq[:, 3], f_min * f_min) | bits_upper(4, sq[:, 3], Gq[:, 3], f_max * f_max)
                sq[:, 4] = guarded(scan(qz - cos2 * qt, depth), Gq[:, 4])
                if tilt_max > 0.0:
                    ct = (sq[:, 4, 0] >= 0.0) & (rng[:, 2, 2, 0] > -GRAVITY)
                    vt = (sq[:, 4, 1] + Gq[:, 4] < 0.0) | (rng[:, 2, 2, 1] + G[:, 2, 2] < -GRAVITY)
                    bits |= (ct.astype(np.int64) | (vt.astype(np.int64) << 1)) << 10
    norm = sq.copy()
    norm[:, :4] = rooted(sq[:, :4])
    peak, verdict = np.zeros((n_traj, 5, 4)), np.zeros(n_traj, dtype=np.int64)
    for b in range(n_traj):
        s0, s1 = int(so[b]), int(so[b + 1])
        if s1 <= s0 or (status is not None and int(status[b]) != SOLVED):
            rng[s0:s1], norm[s0:s1], bits[s0:s1] = 0.0, 0.0, 0
            continue
        peak[b, :, :2] = norm[s0:s1, :, :2].min(axis=0)
        peak[b, :, 2:] = norm[s0:s1, :, 2:].max(axis=0)
        peak[b][np.isnan(norm[s0:s1]).any(axis=(0, 2))] = np.nan
        verdict[b] = (np.bitwise_and.reduce(bits[s0:s1]) & 0x1555) | (np.bitwise_or.reduce(bits[s0:s1]) & 0x2AAA)
    return dict(range=rng, norm=norm, peak=peak, seg_verdict=bits.astype(np.int32), verdict=verdict.astype(np.int32), G=G, Gq=Gq, sq=sq)


def decode(word, test):
    """'certified' / 'violated' / 'undecided' of a verdict word for the test of that name"""
    k = TESTS.index(test)
    c, v = (int(word) >> (2 * k)) & 1, (int(word) >> (2 * k + 1)) & 1
    return "certified" if c else "violated" if v else "undecided"


# ---------------------------------------------------------------------------------------------------------------------------------------
# exact extrema (mpmath)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _extrema(mp, p):
    """(min, max) over u in [0, 1] of the polynomial with ascending mpf coefficients p: the ends and every real root of p' inside.
    A point that is no critical point only adds a value the polynomial takes, so a generous test for 'real' costs nothing."""
    def val(u):
        return mp.polyval(p[::-1], u)
    pts = [mp.mpf(0), mp.mpf(1)]
    d = [k * p[k] for k in range(1, len(p))]
    while d and d[-1] == 0:
        d.pop()
    if len(d) > 1:
        scale = max(abs(x) for x in d)
        d = [x / scale for x in d]
        for steps, extra in ((200, 200), (2000, 2000)):
            try:
                roots = mp.polyroots(d[::-1], maxsteps=steps, extraprec=extra)
                break
            except mp.NoConvergence:
                roots = None
        if roots is None:
            raise RuntimeError("polyroots did not converge")
        for z in roots:
            if abs(mp.im(z)) < mp.mpf(10) ** -20 and -mp.mpf(10) ** -20 < mp.re(z) < 1 + mp.mpf(10) ** -20:
                pts.append(min(mp.mpf(1), max(mp.mpf(0), mp.re(z))))
    vals = [val(u) for u in pts]
    return min(vals), max(vals)


def _mul(mp, p, q):
    out = [mp.mpf(0)] * (len(p) + len(q) - 1)
    for i, x in enumerate(p):
        for j, y in enumerate(q):
            out[i + j] += x * y
    return out


def exact_extrema(r, seg_offsets, times, coeff, tilt_max=TILT_GOLDEN, digits=40):
    """Per segment the exact (min, max) of every quantity of uavqp_envelope_*, as decimal strings of `digits` digits:
    range [sum M][4][3][2] and norm [sum M][5][2] (|v|, |a|, |j|, thrust rooted; w as it is, with the float64 cos^2 of the library)."""
    import mpmath
    mp = mpmath.mp
    mp.dps = 60
    C = segment_coefficients(r, seg_offsets, coeff)
    T = np.asarray(times, dtype=np.float64).ravel()
    cos2 = mp.mpf(math.cos(tilt_max) * math.cos(tilt_max))

    def s(x):
        return mp.nstr(x, digits)

    out_range, out_norm = [], []
    for i in range(C.shape[0]):
        Ti = mp.mpf(float(T[i]))
        polys = {}
        rr = []
        for D in range(4):
            m = 2 * r - 1 - D
            row = []
            for ax in range(3):
                p = [mp.mpf(falling(k + D, D)) * mp.mpf(float(C[i, ax, k + D])) * Ti ** k for k in range(m + 1)]
                polys[D, ax] = p
                row.append([s(x) for x in _extrema(mp, p)])
            rr.append(row)
        out_range.append(rr)
        nn = []
        for D in (1, 2, 3):
            q = [sum(t) for t in zip(*[_mul(mp, polys[D, ax], polys[D, ax]) for ax in range(3)])]
            lo, hi = _extrema(mp, q)
            nn.append([s(mp.sqrt(max(lo, 0))), s(mp.sqrt(hi))])
        z = [polys[2, 0], polys[2, 1], [polys[2, 2][0] + mp.mpf(GRAVITY)] + polys[2, 2][1:]]
        sqs = [_mul(mp, p, p) for p in z]
        qt = [a + b + c for a, b, c in zip(*sqs)]
        lo, hi = _extrema(mp, qt)
        nn.append([s(mp.sqrt(max(lo, 0))), s(mp.sqrt(hi))])
        w = [c - cos2 * t for c, t in zip(sqs[2], qt)]
        nn.append([s(x) for x in _extrema(mp, w)])
        out_norm.append(nn)
    return dict(range=out_range, norm=out_norm)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the recorded cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def solved_trajectory(oracle, r, M, rng):
    """the CPU oracle's exact solve of M segments through random waypoints, T in [0.3, 3]: (T [M], coeff [3 * 2r * M])"""
    wp = np.cumsum(rng.uniform(-2.0, 2.0, size=(M + 1, 3)), axis=0)
    T = rng.uniform(0.3, 3.0, size=M)
    bc = np.zeros((1, 2, r - 1, 3))
    bc[0, 0, 0] = rng.uniform(-1.0, 1.0, size=3)
    coef, st = oracle.solve_exact_batch(r, np.array([0, M], dtype=np.int32), wp, T, bc)
    assert st[0] == 0
    return T, coef


def closed_form(r, kind):
    """one segment, [3][2r] coefficients and its duration"""
    c = np.zeros((3, 2 * r))
    if kind == "constant_velocity":
        c[:, 0], c[:, 1], T = (1.0, -2.0, 0.5), (1.5, -2.0, 0.25), 1.75
    elif kind == "free_fall":
        c[:, 0], c[:, 1], T = (0.0, 1.0, 30.0), (2.0, -1.0, 3.0), 1.25
        c[2, 2] = -GRAVITY / 2.0
    elif kind == "parabola":   # v_x(t) = 1 + 3 t - 5 t^2 peaks with 1.45 at t = 0.3 T: strictly between the ends (1 and -1), on no dyadic point
        T = 1.0
        c[0, 1], c[0, 2], c[0, 3] = 1.0, 1.5, -5.0 / 3.0
    else:
        raise ValueError(kind)
    return np.array([T]), c.ravel()


CLOSED = ("constant_velocity", "free_fall", "parabola")


def cases():
    """name -> dict(r, seg_offsets, times, coeff): the recorded cases (the CPU oracle must be built)"""
    from oracle import oracle
    oracle.build()
    out = {}
    for r in (3, 4):
        rng = np.random.default_rng(4200 + r)
        for M in (1, 3, 9):
            T, c = solved_trajectory(oracle, r, M, rng)
            out[f"r{r}-M{M}"] = dict(r=r, seg_offsets=[0, M], times=T, coeff=c)
        parts = [solved_trajectory(oracle, r, M, rng) if M else (np.zeros(0), np.zeros(0)) for M in (2, 0, 9, 1)]
        out[f"r{r}-ragged"] = dict(r=r, seg_offsets=[0, 2, 2, 11, 12], times=np.concatenate([p[0] for p in parts]),
                                   coeff=np.concatenate([p[1] for p in parts]))
        for kind in CLOSED:
            T, c = closed_form(r, kind)
            out[f"r{r}-{kind}"] = dict(r=r, seg_offsets=[0, 1], times=T, coeff=c)
    return out


def load_golden():
    """name -> dict(r, seg_offsets, times, coeff, exact=dict(range, norm) of mpmath numbers)"""
    import mpmath
    mpmath.mp.dps = 60
    with open(GOLDEN) as fh:
        raw = json.load(fh)
    assert raw["tilt_max"] == TILT_GOLDEN
    out = {}
    for name, rec in raw["cases"].items():
        def conv(x):
            return [conv(y) for y in x] if isinstance(x, list) else mpmath.mpf(x)
        out[name] = dict(r=rec["r"], seg_offsets=np.array(rec["seg_offsets"], dtype=np.int32), times=np.array(rec["times"], dtype=np.float64),
                         coeff=np.array(rec["coeff"], dtype=np.float64), exact=dict(range=conv(rec["range"]), norm=conv(rec["norm"])))
    return out


def sandwich_failures(got, exact, name=""):
    """The soundness of the four numbers of every quantity of one case against the exact extrema, in mpmath arithmetic and WITHOUT a
    tolerance: outer_lo <= min <= inner_lo + G and inner_hi - G <= max <= outer_hi.  The outer pair is the guarantee.  The inner pair is
    a computed value of the polynomial, not an exact one: it enters with the guard G (for a rooted norm Gq / (2 value)), the movement the
    verdict's violated bit applies to it.  got: the arrays of uavqp_envelope_* plus G, Gq (envelope() above).  Returns a list of strings."""
    import mpmath
    f = mpmath.mpf
    bad = []

    def check(tag, quad, lo, hi, g):
        olo, ilo, ihi, ohi = (f(float(x)) for x in quad)
        if not (olo <= lo and hi <= ohi):
            bad.append(f"{name} {tag}: outer [{olo}, {ohi}] does not hold [{lo}, {hi}]")
        if not (lo <= ilo + g and ihi - g <= hi):
            bad.append(f"{name} {tag}: inner [{ilo}, {ihi}] lies outside [{lo}, {hi}] by more than the guard {g}")

    for i in range(got["range"].shape[0]):
        for D in range(4):
            for ax in range(3):
                lo, hi = exact["range"][i][D][ax]
                check(f"seg {i} D={D} axis {ax}", got["range"][i, D, ax], lo, hi, f(float(got["G"][i, D, ax])))
        for k in range(5):
            lo, hi = exact["norm"][i][k]
            g = f(float(got["Gq"][i, k]))
            if k < 4:   # the guard of the square, carried through the root at each end
                quad = got["norm"][i, k]
                glo = g / (2 * f(float(quad[1]))) if quad[1] > 0 else mpmath.sqrt(g)
                ghi = g / (2 * f(float(quad[2]))) if quad[2] > 0 else mpmath.sqrt(g)
                olo, ilo, ihi, ohi = (f(float(x)) for x in quad)
                if not (olo <= lo and hi <= ohi):
                    bad.append(f"{name} seg {i} {NORMS[k]}: outer [{olo}, {ohi}] does not hold [{lo}, {hi}]")
                if not (lo <= ilo + glo and ihi - ghi <= hi):
                    bad.append(f"{name} seg {i} {NORMS[k]}: inner [{ilo}, {ihi}] lies outside [{lo}, {hi}] by more than the guard")
            else:
                check(f"seg {i} w", got["norm"][i, k], lo, hi, g)
    return bad
