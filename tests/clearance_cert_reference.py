"""CPU reference of uavqp_clearance_certificate_* (include/uavqp.h): the method of qp_clearance_cert.h restated line by line in numpy
float64 (certificate), an independent TRUTH (truth: the brute-force distance from a point to the union of the occupied cubes and the
map's outside, every point against every occupied cube), and the inputs the CPU test (tests/test_clearance_cert_reference.py) fixes for
the GPU test (tests/test_gpu_clearance_cert.py): batches on the pillar scene of tests/esdf_scene.py, one d_req per batch.

The bound.  O = the closed cubes of the occupied voxels plus everything outside the map.  res the voxel edge, c_v = origin + (v + 0.5) res,
s_v = res sqrt(sq_pos[v]) (+inf where sq_pos[v] = INT32_MAX).  For a point p and ANY voxel v (the method takes the voxel of p,
floor((p - origin) / res) clamped into the grid):
    dist(p, occupied cubes) >= s_v - (sqrt(3)/2) res - |p - c_v|      every occupied centre is at least s_v from c_v, every point of an
                                                                      occupied cube within (sqrt(3)/2) res of its centre
    dist(p, occupied cubes) <= s_v + |p - c_v| - res/2, 0 if sq_pos[v] = 0    the nearest occupied cube holds the ball of radius res/2
A leaf, the sub-curve over [l, l + 1] T / 2^depth, stays in the box of its D = 0 Bernstein coefficients widened per axis by the envelope's
guard G_x = 16 (n + 1) 2^-53 S_x; m its centre, h its half diagonal, v the voxel of m:
    L_leaf = min( s_v - (sqrt(3)/2) res - |m - c_v| - h, min_x min(lo_x - origin_x, top_x - hi_x) ) - R
Witness points p_l, l = 0..2^depth, are the leaf end coefficients (the curve at t = l T / 2^depth):
    U_l = s_v + |p_l - c_v| - res/2 + sqrt(3) max_x G_x + R,   U_l = sqrt(3) max_x G_x + R  outside the map or in an occupied voxel
    lower = max(0, min L_leaf),  upper = min U_l,  witness = the smallest l that attains it
R = 64 2^-53 (max_x S_x + A), A = max_x max(|origin_x|, |top_x|) + res |dims|: the rounding allowance of the field arithmetic (every
operand is at most max S + A in magnitude, about twenty roundings of 2^-53 each; 64 leaves room).  ALLOWANCE of a segment: sqrt(3) max G + R,
within which two evaluations of these formulas agree."""
import functools
import math

import numpy as np

import envelope_reference as E
import esdf_scene as S

EPS = 2.0 ** -53
INT32_MAX = 2 ** 31 - 1
SQRT3, HALF_SQRT3 = 1.7320508075688772, 0.8660254037844386
CERTIFIED, VIOLATED, OUTSIDE = 1, 2, 4
SOLVED = 1
OUT = ("clear", "witness", "peak", "seg_verdict", "verdict")


def make_map(sq_pos, origin, res):
    """what the kernel sees of a map: sq_pos [nx][ny][nz], origin, top = origin + dims res, res, 1 / res, A"""
    sq_pos = np.asarray(sq_pos, dtype=np.int64)
    origin = np.asarray(origin, dtype=np.float64)
    dims = np.array(sq_pos.shape, dtype=np.int64)
    top = origin + dims.astype(np.float64) * res
    mag = float(max(np.abs(origin).max(), np.abs(top).max())) + res * math.sqrt(float(np.sum(dims * dims)))
    return dict(sq_pos=sq_pos, origin=origin, top=top, dims=dims, res=float(res), inv_res=1.0 / float(res), mag=mag)


def lookup(m, P):
    """P [...][3] -> (s_v, |p - c_v|, sq_pos[v], margin) of the voxel of p clamped into the grid (a NaN coordinate: index 0); margin: the
    smallest distance of a finite (p - origin) / res to an integer"""
    x = (P - m["origin"]) * m["inv_res"]
    f = np.fmin(np.fmax(np.floor(x), 0.0), (m["dims"] - 1).astype(np.float64))
    idx = f.astype(np.int64)
    sq = m["sq_pos"][idx[..., 0], idx[..., 1], idx[..., 2]]
    d = P - (m["origin"] + (f + 0.5) * m["res"])
    off = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    s = np.where(sq == INT32_MAX, np.inf, m["res"] * np.sqrt(sq.astype(np.float64)))
    fin = x[np.isfinite(x)]
    margin = float(np.min(np.abs(fin - np.round(fin)))) if fin.size else 1.0
    return s, off, sq, margin


def leaves_of(b, depth):
    """b [n][nc] -> [n][2^depth][nc]: the leaves in the order of t (leaf l is the sub-curve over [l, l + 1] / 2^depth)"""
    cur = b[:, None, :]
    for _ in range(depth):
        left, right = E.split(cur)
        cur = np.stack([left, right], axis=2).reshape(b.shape[0], -1, b.shape[1])
    return cur


def certificate(r, seg_offsets, times, coeff, m, status=None, depth=4, d_req=0.5):
    """The method of qp_clearance_cert.h on the map m (make_map).  Returns the five outputs of uavqp_clearance_certificate_* and, for the
    tests: allow [sum M] the allowance sqrt(3) max G + R of each segment, margin (the smallest distance of a leaf centre or witness, in
    voxels, to a voxel boundary, and of a witness coordinate, in metres, to a face of the map: no index and no outside flag hangs on a
    rounding), h [sum M] the largest half diagonal of a leaf box, points [sum M][2^depth + 1][3] the witness points."""
    so = np.asarray(seg_offsets, dtype=np.int64)
    n_traj, tot = so.size - 1, int(so[-1])
    nc = 2 * r
    T = np.asarray(times, dtype=np.float64).ravel()
    C = E.segment_coefficients(r, so, coeff)
    o, top, res = m["origin"], m["top"], m["res"]
    with np.errstate(all="ignore"):
        w, S_, G = [], [], []
        for ax in range(3):
            bb, SS = E.bernstein(C[:, ax], T, 0)
            w.append(leaves_of(bb, depth))
            S_.append(SS)
            G.append(16.0 * float(nc) * EPS * SS)
        w, S_, G = np.stack(w, axis=2), np.stack(S_, axis=1), np.stack(G, axis=1)    # [tot][2^depth][3][nc], [tot][3], [tot][3]
        Smax, Gmax = S_.max(axis=1), G.max(axis=1)
        Smax[np.isnan(S_).any(axis=1)] = np.nan
        Gmax[np.isnan(G).any(axis=1)] = np.nan
        R = 64.0 * EPS * (Smax + m["mag"])
        pad = SQRT3 * Gmax + R
        # the guarded box of every leaf
        lo, hi = w.min(axis=3) - G[:, None, :], w.max(axis=3) + G[:, None, :]
        mid, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
        face = np.minimum(lo - o, top - hi).min(axis=2)
        h = np.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2])
        s, off, _, margin = lookup(m, mid)
        L = np.minimum(s - HALF_SQRT3 * res - off - h, face) - R[:, None]
        low = L.min(axis=1)
        # the witnesses: the left end of every leaf and the right end of the last
        P = np.concatenate([w[:, :, :, 0], w[:, -1:, :, nc - 1]], axis=1)
        s, off, sq, margin_w = lookup(m, P)
        outside = ~np.all((P >= o) & (P <= top), axis=2)
        U = np.where(outside | (sq == 0), 0.0, s + off - 0.5 * res) + pad[:, None]
        fin = np.isfinite(P)
        margin_f = float(np.min(np.minimum(np.abs(P - o), np.abs(P - top))[fin])) if fin.any() else 1.0
        bad = ~(R < np.inf)
        U[bad] = np.inf
        wit = np.argmin(U, axis=1)      # (the first of equal ones: the smallest l)
        up = U[np.arange(tot), wit] if tot else np.zeros(0)
        lower, upper = np.where(bad, np.nan, np.maximum(0.0, low)), np.where(bad, np.nan, up)
        bits = ((lower >= d_req) * CERTIFIED) | ((upper < d_req) * VIOLATED) | (outside.any(axis=1) * OUTSIDE)
        bits[bad] = 0
        wit[bad] = 0
    clear = np.stack([lower, upper], axis=1)
    peak, verdict = np.zeros((n_traj, 2)), np.zeros(n_traj, dtype=np.int64)
    for b in range(n_traj):
        s0, s1 = int(so[b]), int(so[b + 1])
        if s1 <= s0 or (status is not None and int(status[b]) != SOLVED):
            clear[s0:s1], wit[s0:s1], bits[s0:s1] = 0.0, 0, 0
            continue
        peak[b] = np.nan if np.isnan(clear[s0:s1]).any() else clear[s0:s1].min(axis=0)
        verdict[b] = (np.bitwise_and.reduce(bits[s0:s1]) & CERTIFIED) | (np.bitwise_or.reduce(bits[s0:s1]) & (VIOLATED | OUTSIDE))
    return dict(clear=clear, witness=wit.astype(np.int32), peak=peak, seg_verdict=bits.astype(np.int32), verdict=verdict.astype(np.int32),
                allow=pad, margin=min(margin, margin_w, margin_f), h=h.max(axis=1) if tot else np.zeros(0), points=P)


def state(word):
    return "certified" if int(word) & CERTIFIED else "violated" if int(word) & VIOLATED else "undecided"


def two_guards_away(ref, d_req):
    """the precondition of verdict parity: d_req is more than two allowances from every lower and upper, and no voxel index or outside
    flag hangs on a rounding (margin in voxels / metres against allowances of 1e-13)"""
    c, a = ref["clear"], ref["allow"]
    live = np.isfinite(c).all(axis=1) & (ref["allow"] > 0)
    return bool(np.all(np.abs(c[live] - d_req) > 2 * a[live, None])) and ref["margin"] >= 1e-9


# ---------------------------------------------------------------------------------------------------------------------------------------
# truth
# ---------------------------------------------------------------------------------------------------------------------------------------
def truth(occ, origin, res, P):
    """P [n][3] -> [n]: the distance from each point to O = (the closed cubes of the occupied voxels) + (everything outside the map), in
    float64, by brute force: every point against every occupied cube (the squared distance to a cube is the sum over the axes of
    max(lo - p, 0, p - hi)^2) and against the six faces.  0 for a point outside the map or inside an occupied cube."""
    occ = np.asarray(occ) != 0
    origin = np.asarray(origin, dtype=np.float64)
    top = origin + np.array(occ.shape, dtype=np.float64) * res
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    vox = np.argwhere(occ)
    out = np.empty(P.shape[0])
    for a in range(0, P.shape[0], 2048):
        p = P[a:a + 2048]
        d_face = np.minimum(p - origin, top - p).min(axis=1)
        d2 = np.zeros((p.shape[0], vox.shape[0]))
        for ax in range(3):
            lo = origin[ax] + vox[:, ax].astype(np.float64) * res
            d = np.maximum(np.maximum(lo[None, :] - p[:, ax, None], p[:, ax, None] - (lo[None, :] + res)), 0.0)
            d2 += d * d
        d_occ = np.sqrt(d2.min(axis=1)) if vox.shape[0] else np.full(p.shape[0], np.inf)
        out[a:a + 2048] = np.maximum(0.0, np.minimum(d_face, d_occ))
    return out


def curve(r, seg_offsets, times, coeff, n_per_seg):
    """-> [sum M][n_per_seg + 1][3]: every segment by Horner at t = k T / n_per_seg, k = 0..n_per_seg (independent of the Bernstein form)"""
    C = E.segment_coefficients(r, seg_offsets, coeff)
    T = np.asarray(times, dtype=np.float64).ravel()
    t = T[:, None] * (np.arange(n_per_seg + 1) / float(n_per_seg))[None, :]
    out = np.zeros((C.shape[0], n_per_seg + 1, 3))
    for k in range(2 * r - 1, -1, -1):
        out = out * t[:, :, None] + C[:, None, :, k]
    return out


def soundness_failures(res, depth, tr, tag=""):
    """res: the outputs of a certificate at `depth`; tr [sum M][n_per_seg + 1] the truth along curve(.., n_per_seg), n_per_seg a multiple
    of 2^depth (the witnesses are then among the samples).  -> list of strings, empty when  lower <= min truth  and
    truth(witness) <= upper  on every segment with finite bounds"""
    bad = []
    n_per_seg = tr.shape[1] - 1
    step = n_per_seg >> depth
    assert step << depth == n_per_seg
    for i in range(tr.shape[0]):
        lo, up = res["clear"][i]
        if not (np.isfinite(lo) and (lo != 0 or up != 0 or res["seg_verdict"][i] != 0)):
            continue
        if not lo <= tr[i].min():
            bad.append(f"{tag} segment {i}: lower {lo!r} > min truth {tr[i].min()!r}")
        at = tr[i, int(res["witness"][i]) * step]
        if not at <= up:
            bad.append(f"{tag} segment {i}: truth at witness {int(res['witness'][i])} = {at!r} > upper {up!r}")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------------
# the inputs of the tests
# ---------------------------------------------------------------------------------------------------------------------------------------
DEPTHS = (0, 2, 3, 4, 6)          # below, at and above the three levels the lanes of a group share out
D_REQ = {"flight": 0.3, "ragged": 0.25, "uniform9": 0.3, "uniform70": 0.35}     # one per batch; checked by test_clearance_cert_reference.py
SEEDS = {"flight": 61, "ragged": 62, "uniform9": 63, "uniform70": 64}
N_TRUTH = 512                     # samples per segment of the soundness tests: 64 per leaf at depth 3, 8 at depth 6


def batch(kind, r):
    """flight: esdf_scene.flight_batch, ragged (64 trajectories, M in {1, 2, 3, 5}; every eighth flies out of the map);
    ragged: 12 trajectories with M in {1, 2, 5, 9} by the same walks at steps of 0.4 .. 0.8 m (the eighth flies out);
    uniform9 / uniform70: 9 (one past the eight groups of a wave) / 70 trajectories of 4 segments, no offsets"""
    seed = SEEDS[kind] + 10 * r
    if kind == "flight":
        return S.flight_batch(r, False, seed)
    rng = np.random.default_rng(seed)
    if kind == "ragged":
        return S._flights(rng, np.array([1, 2, 5, 9] * 3), r, False, step_lo=0.4, step_hi=0.8)
    return S._flights(rng, np.full({"uniform9": 9, "uniform70": 70}[kind], 4), r, True)


def head(b, n):
    """the first n trajectories of a batch"""
    so = b["so"][:n + 1]
    tot = int(so[-1])
    return dict(b, n=n, so=so, wp=b["wp"][:tot + n], T=b["T"][:tot], bc=b["bc"][:n], mmax=int(np.diff(so).max()))


def single(b, coeff, t):
    """trajectory t of a batch alone -> (seg_offsets [2], times, coeff)"""
    s0, s1, nc3 = int(b["so"][t]), int(b["so"][t + 1]), 3 * 2 * b["r"]
    return np.array([0, s1 - s0], dtype=np.int32), b["T"][s0:s1], np.asarray(coeff)[nc3 * s0:nc3 * s1]


DEEP = 3        # the trajectory of the ragged batch (M = 9) that depth 8 runs on


@functools.lru_cache(maxsize=None)
def scene_map():
    occ, ref = S.scene_reference()
    return occ, make_map(ref["sq_pos"], S.ORIGIN, S.MRES)


def scene_truth(r, so, T, coeff, n_per_seg=N_TRUTH):
    occ, _ = scene_map()
    pts = curve(r, so, T, coeff, n_per_seg)
    return truth(occ, S.ORIGIN, S.MRES, pts.reshape(-1, 3)).reshape(pts.shape[:2])
