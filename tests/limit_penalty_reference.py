"""A designed reference of the velocity / acceleration limit penalty (include/uavqp.h, uavqp_limit_penalty_device) in numpy longdouble.

Not a port of the kernel: every sample evaluates its derivatives as PLAIN POWER SUMS  p^(d)(t) = sum_k k! / (k - d)! c_k t^(k - d)  from a
table of monomial values (no Horner recurrence), the gradient in the coefficients is assembled from the same monomial table by the chain
rule written out per sample, and all sums are longdouble.

    Phi = sum_i (T_i / K) sum_{s=0..K} om_s [ w_v pos(|v|^2 / v_max^2 - 1)^3 + w_a pos(|a|^2 / a_max^2 - 1)^3 ]   at t = (s / K) T_i

penalty(...) -> dict with
    phi         [n_traj]       Phi per trajectory
    grad_coeff  layout of coeff ([axis][segment][2r] per trajectory): dPhi/dc at fixed durations
    grad_times  [sum M]        explicit dPhi/dT_i at fixed coefficients
    peak        [n_traj][2]    largest sampled |v| / v_max, |a| / a_max
all longdouble."""
import math

import numpy as np

LD = np.longdouble
DEFAULTS = dict(samples_per_seg=8, v_max=7.0, a_max=10.0, weight_v=1e3, weight_a=1e3)


def _monomials(nc, d, t):
    """t [...] -> [..., nc]: d/dt^d of t^k, k! / (k - d)! t^(k - d), zero for k < d (longdouble)"""
    out = np.zeros(t.shape + (nc,), dtype=LD)
    for k in range(d, nc):
        out[..., k] = LD(math.factorial(k) // math.factorial(k - d)) * t ** (k - d)
    return out


def trajectory(c, T, samples_per_seg, v_max, a_max, weight_v, weight_a):
    """c [3][M][nc], T [M] -> (Phi_i [M], dPhi_i/dc [3][M][nc], explicit dPhi_i/dT_i [M], max |v|^2, max |a|^2); all samples at once"""
    c = np.asarray(c, dtype=LD)
    T = np.asarray(T, dtype=LD)
    K = int(samples_per_seg)
    nc = c.shape[2]
    v2, a2, wv, wa = LD(v_max) ** 2, LD(a_max) ** 2, LD(weight_v), LD(weight_a)
    tau = np.arange(K + 1, dtype=LD) / LD(K)                  # [S]
    om = np.ones(K + 1, dtype=LD)
    om[0] = om[K] = LD(0.5)
    t = T[:, None] * tau[None, :]                             # [M][S]
    m1, m2, m3 = _monomials(nc, 1, t), _monomials(nc, 2, t), _monomials(nc, 3, t)      # [M][S][nc]
    v, a, j = (np.einsum("xmk,msk->xms", c, m) for m in (m1, m2, m3))                    # [3][M][S]
    vv, aa = (v * v).sum(axis=0), (a * a).sum(axis=0)          # [M][S]
    pv, pa = np.maximum(LD(0), vv / v2 - 1), np.maximum(LD(0), aa / a2 - 1)
    h = T / LD(K)
    phi = (om * (wv * pv ** 3 + wa * pa ** 3)).sum(axis=1)     # [M], before the factor T / K
    # d(pos^3) = 3 pos^2 d(ratio); d|v|^2 / dc_{x,k} = 2 v_x m1_k; d|v|^2 / dt = 2 v.a, dt / dT = tau
    dv, da = 3 * wv * pv ** 2 / v2, 3 * wa * pa ** 2 / a2
    g = np.einsum("ms,xms,msk->xmk", om * dv, 2 * v, m1) + np.einsum("ms,xms,msk->xmk", om * da, 2 * a, m2)
    d_expl = (om * tau * (dv * 2 * (v * a).sum(axis=0) + da * 2 * (a * j).sum(axis=0))).sum(axis=1)
    return h * phi, h[None, :, None] * g, phi / LD(K) + h * d_expl, vv.max(), aa.max()


def penalty(r, seg_offsets, times, coeff, status=None, solved_value=1, **limits):
    p = dict(DEFAULTS, **limits)
    so = np.asarray(seg_offsets, dtype=np.int64)
    times = np.asarray(times).ravel()
    coeff = np.asarray(coeff).ravel()
    n, nc = so.size - 1, 2 * r
    out = dict(phi=np.zeros(n, dtype=LD), grad_coeff=np.zeros(coeff.size, dtype=LD), grad_times=np.zeros(times.size, dtype=LD),
               peak=np.zeros((n, 2), dtype=LD))
    for b in range(n):
        s0, s1 = int(so[b]), int(so[b + 1])
        M = s1 - s0
        if M < 1 or (status is not None and int(status[b]) != solved_value):
            continue
        c = coeff[3 * nc * s0:3 * nc * s1].reshape(3, M, nc)
        phi_i, g, dT, vv_max, aa_max = trajectory(c, times[s0:s1], p["samples_per_seg"], p["v_max"], p["a_max"], p["weight_v"], p["weight_a"])
        out["phi"][b] = phi_i.sum()
        out["grad_coeff"][3 * nc * s0:3 * nc * s1] = g.ravel()
        out["grad_times"][s0:s1] = dT
        out["peak"][b] = (np.sqrt(vv_max) / LD(p["v_max"]), np.sqrt(aa_max) / LD(p["a_max"]))
    return out


def phi_only(r, seg_offsets, times, coeff, **limits):
    """[n_traj] Phi as float64 (for objectives assembled on the CPU)"""
    return penalty(r, seg_offsets, times, coeff, **limits)["phi"].astype(np.float64)
