"""A designed reference of the attitude penalty (include/uavqp.h, uavqp_attitude_penalty_device) in numpy longdouble.

Not a port of the kernel: every sample evaluates its derivatives as plain power sums from a table of monomial values (no Horner
recurrence), |z x j|^2 is taken from the identity f2 |j|^2 - (z.j)^2 the header states (the kernel forms the cross product), the gradient in
the coefficients is assembled from the monomial tables by the chain rule written out per sample, and all sums are longdouble.

    z = a + gravity e_z, f2 = |z|^2, kappa = tan^2(tilt_max), pos(x) = max(0, x)
    u_hi = f2 / f_max^2 - 1,   u_lo = 1 - f2 / f_min^2 (absent when f_min = 0)
    u_tilt = (z_x^2 + z_y^2 - kappa z_z |z_z|) / gravity^2
    u_rate = (f2 |j|^2 - (z.j)^2 - rate_max^2 f2^2) / (rate_max^2 gravity^4)
    phi = w_thrust (pos(u_hi)^3 + pos(u_lo)^3) + w_tilt pos(u_tilt)^3 + w_rate pos(u_rate)^3
    Phi = sum_i (T_i / K) sum_{s=0..K} om_s phi(t = (s / K) T_i)

penalty(...) -> dict with
    phi         [n_traj]       Phi per trajectory
    grad_coeff  layout of coeff ([axis][segment][2r] per trajectory): dPhi/dc at fixed durations
    grad_times  [sum M]        explicit dPhi/dT_i at fixed coefficients
    peak        [n_traj][4]    largest |z|, smallest |z|, largest tilt angle, largest body rate over the samples ({0, inf, 0, 0} without one)
    terms       [n_traj][3]    Phi split into its thrust, tilt and rate parts
all longdouble."""
import numpy as np

from limit_penalty_reference import _monomials

LD = np.longdouble
DEFAULTS = dict(samples_per_seg=8, gravity=9.81, f_min=3.0, f_max=20.0, tilt_max=1.05, rate_max=2.1, weight_thrust=1e3, weight_tilt=1e3,
                weight_rate=1e3)
NO_SAMPLE = (0.0, np.inf, 0.0, 0.0)


def trajectory(c, T, p):
    """c [3][M][nc], T [M] -> (Phi_i [M], dPhi_i/dc [3][M][nc], explicit dPhi_i/dT_i [M], peaks (4), terms (3)); all samples at once"""
    c = np.asarray(c, dtype=LD)
    T = np.asarray(T, dtype=LD)
    K = int(p["samples_per_seg"])
    nc = c.shape[2]
    g, fmin, fmax, rate = LD(p["gravity"]), LD(p["f_min"]), LD(p["f_max"]), LD(p["rate_max"])
    kappa = np.tan(LD(p["tilt_max"])) ** 2
    wth, wti, wr = LD(p["weight_thrust"]), LD(p["weight_tilt"]), LD(p["weight_rate"])
    tau = np.arange(K + 1, dtype=LD) / LD(K)
    om = np.ones(K + 1, dtype=LD)
    om[0] = om[K] = LD(0.5)
    t = T[:, None] * tau[None, :]                                     # [M][S]
    m2, m3, m4 = _monomials(nc, 2, t), _monomials(nc, 3, t), _monomials(nc, 4, t)
    a, j, s = (np.einsum("xmk,msk->xms", c, m) for m in (m2, m3, m4))   # [3][M][S]
    z = a.copy()
    z[2] += g
    f2, jj, zj = (z * z).sum(axis=0), (j * j).sum(axis=0), (z * j).sum(axis=0)
    hh = z[0] ** 2 + z[1] ** 2
    rg4 = rate ** 2 * g ** 4
    u_hi = f2 / fmax ** 2 - 1
    u_lo = 1 - f2 / fmin ** 2 if fmin > 0 else np.full_like(f2, -1)
    u_tilt = (hh - kappa * z[2] * np.abs(z[2])) / g ** 2
    u_rate = (f2 * jj - zj ** 2 - rate ** 2 * f2 ** 2) / rg4
    ph, pl, pt, pr = (np.maximum(LD(0), u) for u in (u_hi, u_lo, u_tilt, u_rate))
    parts = np.stack([wth * (ph ** 3 + pl ** 3), wti * pt ** 3, wr * pr ** 3])        # [3][M][S]
    h = T / LD(K)
    terms = ((om * parts).sum(axis=2) * h).sum(axis=1)
    phi = (om * parts.sum(axis=0)).sum(axis=1)                        # [M], before the factor T / K
    zero = np.zeros_like(f2)
    G_a = 3 * wth * (ph ** 2 * 2 * z / fmax ** 2 - (pl ** 2 * 2 * z / fmin ** 2 if fmin > 0 else 0)) \
        + 3 * wti * pt ** 2 * np.stack([2 * z[0], 2 * z[1], -2 * kappa * np.abs(z[2])]) / g ** 2 \
        + 3 * wr * pr ** 2 * (2 * jj * z - 2 * zj * j - 4 * rate ** 2 * f2 * z) / rg4
    G_j = 3 * wr * pr ** 2 * (2 * f2 * j - 2 * zj * z) / rg4 + zero
    gc = np.einsum("s,xms,msk->xmk", om, G_a, m2) + np.einsum("s,xms,msk->xmk", om, G_j, m3)
    d_expl = (om * tau * ((G_a * j).sum(axis=0) + (G_j * s).sum(axis=0))).sum(axis=1)
    # peaks, in physical units
    f = np.sqrt(f2)
    tilt = np.arctan2(np.sqrt(hh), z[2])
    x = np.stack([z[1] * j[2] - z[2] * j[1], z[2] * j[0] - z[0] * j[2], z[0] * j[1] - z[1] * j[0]])
    ok = f2 > 0
    rate_s = np.where(ok, np.sqrt((x * x).sum(axis=0)) / np.where(ok, f2, 1), 0)
    peaks = (f.max(), f.min(), tilt.max(), rate_s.max())
    return h * phi, h[None, :, None] * gc, phi / LD(K) + h * d_expl, peaks, terms


def penalty(r, seg_offsets, times, coeff, status=None, solved_value=1, **params):
    p = dict(DEFAULTS, **params)
    so = np.asarray(seg_offsets, dtype=np.int64)
    times = np.asarray(times).ravel()
    coeff = np.asarray(coeff).ravel()
    n, nc = so.size - 1, 2 * r
    out = dict(phi=np.zeros(n, dtype=LD), grad_coeff=np.zeros(coeff.size, dtype=LD), grad_times=np.zeros(times.size, dtype=LD),
               peak=np.tile(np.array(NO_SAMPLE, dtype=LD), (n, 1)), terms=np.zeros((n, 3), dtype=LD))
    for b in range(n):
        s0, s1 = int(so[b]), int(so[b + 1])
        M = s1 - s0
        if M < 1 or (status is not None and int(status[b]) != solved_value):
            continue
        c = coeff[3 * nc * s0:3 * nc * s1].reshape(3, M, nc)
        phi_i, g, dT, peaks, terms = trajectory(c, times[s0:s1], p)
        out["phi"][b] = phi_i.sum()
        out["grad_coeff"][3 * nc * s0:3 * nc * s1] = g.ravel()
        out["grad_times"][s0:s1] = dT
        out["peak"][b] = peaks
        out["terms"][b] = terms
    return out


def phi_only(r, seg_offsets, times, coeff, **params):
    """[n_traj] Phi as float64 (for objectives assembled on the CPU)"""
    return penalty(r, seg_offsets, times, coeff, **params)["phi"].astype(np.float64)
