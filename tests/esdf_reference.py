"""A designed reference of the distance-field layer (include/uavqp.h: uavqp_esdf_* and uavqp_clearance_penalty_device), numpy only,
written from the semantics stated in the header and not from the kernels.

  * squared distances by BRUTE FORCE: every voxel against every occupied (free) voxel, in integers -- no separable passes, no envelope;
    and, for grids the brute force cannot afford, by one exact min-plus pass per axis over every pair of a line (separable_sq);
  * the field, the rasteriser, the trilinear query and the penalty in np.longdouble;
  * every query point comes with its MARGIN in voxels: the smallest distance of (pos - origin) / res - 0.5 to an integer on any axis
    (the faces across which the trilinear gradient jumps) and of the position to the two 1e-4 map bounds; the penalty also reports the
    smallest |d - d_safe| over its samples.  Tests that compare gradients assert on these that no sample sits on a discontinuity.
"""
import math

import numpy as np

LD = np.longdouble
INT32_MAX = 2 ** 31 - 1
DEFAULTS = dict(samples_per_seg=8, d_safe=0.5, weight=1e3)


def brute_sq(mask):
    """mask [nx][ny][nz] bool -> int64 [nx][ny][nz]: squared voxel distance to the nearest True voxel, INT32_MAX if there is none.
    Every voxel that is not itself True is compared with every True voxel (a True voxel is its own nearest: 0)."""
    mask = np.asarray(mask, dtype=bool)
    out = np.full(mask.shape, INT32_MAX, dtype=np.int64)
    src = np.argwhere(mask).astype(np.int64)            # [S][3]
    if src.shape[0] == 0:
        return out
    out[mask] = 0
    rest = np.argwhere(~mask).astype(np.int64)
    flat = out.reshape(-1)
    at = np.ravel_multi_index(rest.T, mask.shape) if rest.shape[0] else np.zeros(0, dtype=np.int64)
    chunk = max(1, (1 << 21) // src.shape[0])
    for a in range(0, rest.shape[0], chunk):
        q = rest[a:a + chunk]
        d2 = (q[:, None, 0] - src[None, :, 0]) ** 2 + (q[:, None, 1] - src[None, :, 1]) ** 2 + (q[:, None, 2] - src[None, :, 2]) ** 2
        flat[at[a:a + chunk]] = d2.min(axis=1)
    return out


def separable_sq(mask):
    """The same function as brute_sq by the separability of the squared Euclidean distance: with f = 0 on True voxels and "none"
    elsewhere, one exact pass  out[p] = min_q f[q] + (p - q)^2  along each axis in turn.  int64; every q of a line is visited for every p
    (no early exit, no tiling), so the cost is (the sum of the dimensions) x (the voxels) and a grid too large for brute_sq stays cheap.
    "None" is 2^40 between the passes: above every true value (< 3 * 2^20) plus every (p - q)^2, far below the int64 range."""
    mask = np.asarray(mask, dtype=bool)
    none = np.int64(1) << 40
    f = np.where(mask, np.int64(0), none)
    for axis in range(3):
        g = np.moveaxis(f, axis, 0)
        p = np.arange(g.shape[0], dtype=np.int64).reshape(-1, 1, 1)
        out = np.full(g.shape, none, dtype=np.int64)
        for q in range(g.shape[0]):
            np.minimum(out, g[q][None] + (p - q) ** 2, out=out)
        f = np.moveaxis(out, 0, axis)
    return np.where(f >= none, np.int64(INT32_MAX), f)


SQ = {"brute": brute_sq, "separable": separable_sq}


def field(occ, resolution, max_dist, sq="brute"):
    """occ [nx][ny][nz] (non-zero = occupied) -> dict sq_pos, sq_neg (int64), d_pos, d_neg, dist (longdouble); sq names the function
    that gives the squared distances: "brute" (brute_sq) or "separable" (separable_sq)"""
    occ = np.asarray(occ) != 0
    sq_pos, sq_neg = SQ[sq](occ), SQ[sq](~occ)
    res, md = LD(resolution), LD(max_dist)
    d_pos = np.minimum(res * np.sqrt(sq_pos.astype(LD)), md)
    d_neg = np.minimum(res * np.sqrt(sq_neg.astype(LD)), md)
    dist = np.where(d_neg == 0, d_pos, d_pos - d_neg + res)
    return dict(sq_pos=sq_pos, sq_neg=sq_neg, d_pos=d_pos, d_neg=d_neg, dist=dist)


def rasterize(dims, origin, resolution, points, inflate_xy, inflate_z, occ=None):
    """-> (occ uint8 [nx][ny][nz], margin): margin = the smallest distance of any (p + k res - origin) / res to an integer"""
    dims = tuple(int(d) for d in dims)
    occ = np.zeros(dims, dtype=np.uint8) if occ is None else np.array(occ, dtype=np.uint8)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3).astype(LD)
    res, inv, org = LD(resolution), LD(1) / LD(resolution), np.asarray(origin, dtype=np.float64).astype(LD)
    margin = LD(1)
    for kx in range(-inflate_xy, inflate_xy + 1):
        for ky in range(-inflate_xy, inflate_xy + 1):
            for kz in range(-inflate_z, inflate_z + 1):
                u = (pts + np.array([kx, ky, kz], dtype=LD) * res - org) * inv
                if u.size:
                    margin = min(margin, np.abs(u - np.rint(u)).min())
                idx = np.floor(u).astype(np.int64)
                ok = np.all((idx >= 0) & (idx < np.array(dims)), axis=1)
                occ[idx[ok, 0], idx[ok, 1], idx[ok, 2]] = 1
    return occ, margin


def query(dist, origin, resolution, points):
    """dist [nx][ny][nz] (any float type) -> dict dist [n], grad [n][3], inside [n] uint8, margin [n] (voxels), scale [n] (largest |corner|)"""
    D = np.asarray(dist).astype(LD)
    dims = np.array(D.shape, dtype=np.int64)
    pts = np.asarray(points).reshape(-1, 3).astype(LD)
    n = pts.shape[0]
    res, inv, org = LD(resolution), LD(1) / LD(resolution), np.asarray(origin, dtype=np.float64).astype(LD)
    lo, hi = org + LD(1e-4), org + dims.astype(LD) * res - LD(1e-4)
    inside = np.all((pts >= lo) & (pts <= hi), axis=1)
    margin = np.minimum(np.abs(pts - lo), np.abs(pts - hi)).min(axis=1) * inv
    u = (pts - LD(0.5) * res - org) * inv
    idx = np.floor(u).astype(np.int64)
    face = np.abs(u - np.rint(u)).min(axis=1)
    margin = np.where(inside, np.minimum(margin, face), margin)
    diff = (pts - ((idx.astype(LD) + LD(0.5)) * res + org)) * inv
    out = dict(dist=np.zeros(n, dtype=LD), grad=np.zeros((n, 3), dtype=LD), inside=inside.astype(np.uint8), margin=margin,
               scale=np.zeros(n, dtype=LD))
    v = np.zeros((2, 2, 2, n), dtype=LD)
    for x in range(2):
        for y in range(2):
            for z in range(2):
                c = np.clip(idx + np.array([x, y, z]), 0, dims - 1)
                v[x, y, z] = D[c[:, 0], c[:, 1], c[:, 2]]
    dx, dy, dz = diff[:, 0], diff[:, 1], diff[:, 2]
    v00 = (1 - dx) * v[0, 0, 0] + dx * v[1, 0, 0]
    v01 = (1 - dx) * v[0, 0, 1] + dx * v[1, 0, 1]
    v10 = (1 - dx) * v[0, 1, 0] + dx * v[1, 1, 0]
    v11 = (1 - dx) * v[0, 1, 1] + dx * v[1, 1, 1]
    v0 = (1 - dy) * v00 + dy * v10
    v1 = (1 - dy) * v01 + dy * v11
    d = (1 - dz) * v0 + dz * v1
    gz = (v1 - v0) * inv
    gy = ((1 - dz) * (v10 - v00) + dz * (v11 - v01)) * inv
    gx = ((1 - dz) * (1 - dy) * (v[1, 0, 0] - v[0, 0, 0]) + (1 - dz) * dy * (v[1, 1, 0] - v[0, 1, 0])
          + dz * (1 - dy) * (v[1, 0, 1] - v[0, 0, 1]) + dz * dy * (v[1, 1, 1] - v[0, 1, 1])) * inv
    out["dist"][inside] = d[inside]
    out["grad"][inside] = np.stack([gx, gy, gz], axis=1)[inside]
    out["scale"] = np.abs(v).reshape(8, n).max(axis=0)
    return out


def _monomials(nc, d, t):
    """t [...] -> [..., nc]: d/dt^d of t^k (longdouble)"""
    out = np.zeros(t.shape + (nc,), dtype=LD)
    for k in range(d, nc):
        out[..., k] = LD(math.factorial(k) // math.factorial(k - d)) * t ** (k - d)
    return out


def penalty(r, seg_offsets, times, coeff, dist, origin, resolution, max_dist, status=None, solved_value=1, **params):
    """-> dict phi [n], grad_coeff (layout of coeff), grad_times [sum M], min_dist [n], outside [n] int64 (all longdouble but outside),
    margin (smallest query margin over all samples, voxels), gap (smallest |d - d_safe| over the samples inside the map)"""
    p = dict(DEFAULTS, **params)
    K, d_safe, weight = int(p["samples_per_seg"]), LD(p["d_safe"]), LD(p["weight"])
    so = np.asarray(seg_offsets, dtype=np.int64)
    times = np.asarray(times).ravel()
    coeff = np.asarray(coeff).ravel()
    n, nc = so.size - 1, 2 * r
    out = dict(phi=np.zeros(n, dtype=LD), grad_coeff=np.zeros(coeff.size, dtype=LD), grad_times=np.zeros(times.size, dtype=LD),
               min_dist=np.full(n, LD(max_dist), dtype=LD), outside=np.zeros(n, dtype=np.int64), margin=LD(np.inf), gap=LD(np.inf))
    tau = np.arange(K + 1, dtype=LD) / LD(K)
    om = np.ones(K + 1, dtype=LD)
    om[0] = om[K] = LD(0.5)
    for b in range(n):
        s0, s1 = int(so[b]), int(so[b + 1])
        M = s1 - s0
        if M < 1 or (status is not None and int(status[b]) != solved_value):
            continue
        c = coeff[3 * nc * s0:3 * nc * s1].reshape(3, M, nc).astype(LD)
        T = times[s0:s1].astype(LD)
        t = T[:, None] * tau[None, :]                                      # [M][S]
        m0, m1 = _monomials(nc, 0, t), _monomials(nc, 1, t)                # [M][S][nc]
        pos = np.einsum("xmk,msk->msx", c, m0)                             # [M][S][3]
        vel = np.einsum("xmk,msk->msx", c, m1)
        q = query(dist, origin, resolution, pos.reshape(-1, 3))
        ins = q["inside"].reshape(M, K + 1).astype(bool)
        d = q["dist"].reshape(M, K + 1)
        g = q["grad"].reshape(M, K + 1, 3)
        out["margin"] = min(out["margin"], q["margin"].min())
        out["outside"][b] = int((~ins).sum())
        if ins.any():
            out["min_dist"][b] = d[ins].min()
            out["gap"] = min(out["gap"], np.abs(d[ins] - d_safe).min())
        x = np.where(ins, np.maximum(LD(0), (d_safe - d) / d_safe), LD(0))
        h = T / LD(K)
        phi = (om * weight * x ** 3).sum(axis=1)                            # [M], before the factor T / K
        e = -3 * weight * x ** 2 / d_safe                                   # [M][S]
        gc = np.einsum("ms,msx,msk->xmk", om * e, g, m0)
        d_expl = (om * tau * e * (g * vel).sum(axis=2)).sum(axis=1)
        out["phi"][b] = (h * phi).sum()
        out["grad_coeff"][3 * nc * s0:3 * nc * s1] = (h[None, :, None] * gc).ravel()
        out["grad_times"][s0:s1] = phi / LD(K) + h * d_expl
    return out
