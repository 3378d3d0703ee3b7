"""Reference and inputs for the tests of uavqp_time_reallocate_device (include/uavqp.h): tests/test_time_realloc_contract.py (CPU)
and tests/test_gpu_time_realloc.py.  Nothing here touches a GPU.

reference()            the header's rule restated in np.longdouble, plain power sums, vectorised over the segments of a batch
kernel_arithmetic()    the kernel's own float64 evaluation order (Horner, t = T * s / samples, running maxima) in numpy
designed_cases(r)      synthetic coefficient arrays with a known class per trajectory (the kernel does not care whether they solve anything)
big_ragged_case()      65 536 + 11 trajectories of 1..3 segments, r = 3: past one grid of num_cus * 32 blocks of 8, not a multiple of 8

Coefficient layout (include/uavqp.h): trajectory b starts at 3 * 2r * seg_offsets[b], inside it [axis][segment][2r], ascending powers.
"""
import functools

import numpy as np

LD = np.longdouble
V_MAX, A_MAX, SAMPLES, MAX_STRETCH = 8.0, 4.0, 16, 1.5     # the limits every designed input is scaled against
DEAD_BAND, OVERSHOOT = 1.01, 1.02                           # uavqp_default_settings
M_POOL = (1, 2, 7, 8, 9, 15, 16, 17, 33, 63)
# one wave holds 8 trajectories (8 lanes each): S = designed to stretch, U = designed to stay; every S has a U on both sides in its wave
WAVE_PATTERN = "USUSUUSU"


def offsets_of(n_traj, uniform, seg_offsets):
    return np.arange(n_traj + 1, dtype=np.int64) * uniform if uniform > 0 else np.asarray(seg_offsets, dtype=np.int64)


def segment_view(r, so, coeff):
    """coeff as [total segments][3][2r] (a gathered copy) and the trajectory of every segment."""
    nc = 2 * r
    n = so.size - 1
    M = np.diff(so)
    traj = np.repeat(np.arange(n), M)
    local = np.arange(int(so[-1])) - so[traj]
    base = 3 * nc * so[traj][:, None] + (np.arange(3)[None, :] * M[traj][:, None] + local[:, None]) * nc
    return np.asarray(coeff)[base[:, :, None] + np.arange(nc)[None, None, :]], traj


def _peaks_longdouble(r, C, T, samples, chunk=8192):
    """max over the samples of |v|^2 and |a|^2 per segment; plain sums of powers in longdouble; a non-finite sample gives NaN or Inf."""
    nc = 2 * r
    tot = T.size
    v2 = np.empty(tot, dtype=LD)
    a2 = np.empty(tot, dtype=LD)
    frac = np.arange(samples + 1, dtype=LD) / LD(samples)
    with np.errstate(all="ignore"):
        for lo in range(0, tot, chunk):
            c = C[lo:lo + chunk].astype(LD)
            t = T[lo:lo + chunk].astype(LD)[:, None] * frac[None, :]             # [seg][sample]
            v = np.zeros((c.shape[0], 3, samples + 1), dtype=LD)
            a = np.zeros_like(v)
            for j in range(1, nc):
                v += LD(j) * c[:, :, j, None] * t[:, None, :] ** (j - 1)
            for j in range(2, nc):
                a += LD(j * (j - 1)) * c[:, :, j, None] * t[:, None, :] ** (j - 2)
            v2[lo:lo + chunk] = np.max(np.sum(v * v, axis=1), axis=1)            # np.max / np.maximum propagate NaN
            a2[lo:lo + chunk] = np.max(np.sum(a * a, axis=1), axis=1)
    return v2, a2


def reference(r, n_traj, uniform, seg_offsets, times, coeff, v_max=V_MAX, a_max=A_MAX, samples=SAMPLES, max_stretch=MAX_STRETCH,
              dead_band=DEAD_BAND, overshoot=OVERSHOOT):
    """The rule of include/uavqp.h.  Returns dict(T_new longdouble [sum M], changed int32 [n], rho, rho_v, rho_a longdouble [n],
    factor longdouble [n] (1 where nothing changes), stretched bool [n])."""
    so = offsets_of(n_traj, uniform, seg_offsets)
    T = np.asarray(times, dtype=np.float64).ravel()
    C, traj = segment_view(r, so, coeff)
    v2s, a2s = _peaks_longdouble(r, C, T, samples)
    with np.errstate(all="ignore"):
        v2 = np.maximum.reduceat(v2s, so[:-1])
        a2 = np.maximum.reduceat(a2s, so[:-1])
        rho_v = np.sqrt(v2) / LD(v_max)
        rho_a = np.sqrt(np.sqrt(a2) / LD(a_max))
        rho = np.maximum(rho_v, rho_a)
        stretched = np.isfinite(rho) & (rho > LD(dead_band))
        factor = np.where(stretched, np.minimum(LD(overshoot) * rho, LD(max_stretch)), LD(1))
    return dict(T_new=T.astype(LD) * factor[traj], changed=np.where(stretched, np.diff(so), 0).astype(np.int32), rho=rho, rho_v=rho_v,
                rho_a=rho_a, factor=factor, stretched=stretched)


def kernel_arithmetic(r, n_traj, uniform, seg_offsets, times, coeff, v_max=V_MAX, a_max=A_MAX, samples=SAMPLES, max_stretch=MAX_STRETCH,
                      dead_band=DEAD_BAND, overshoot=OVERSHOOT):
    """realloc_kernel's float64 arithmetic in its own order: t = T * s / samples, Horner from the highest power with the factors j and
    j (j - 1) folded into the coefficients, squares summed x, y, z, running maxima, ratio, one factor, T * factor.  (The kernel fuses each
    Horner step into one fma; numpy rounds the product and the sum separately -- one more rounding of the same size per step.)
    Returns (T_new float64, changed int32)."""
    nc = 2 * r
    so = offsets_of(n_traj, uniform, seg_offsets)
    T = np.asarray(times, dtype=np.float64).ravel()
    C, traj = segment_view(r, so, coeff)
    v2s = np.zeros(T.size)
    a2s = np.zeros(T.size)
    with np.errstate(all="ignore"):
        for s in range(samples + 1):
            t = T * float(s) / float(samples)
            vs = np.zeros(T.size)
            acs = np.zeros(T.size)
            for ax in range(3):
                v = np.zeros(T.size)
                ac = np.zeros(T.size)
                for j in range(nc - 1, 0, -1):
                    v = v * t + float(j) * C[:, ax, j]
                for j in range(nc - 1, 1, -1):
                    ac = ac * t + float(j * (j - 1)) * C[:, ax, j]
                vs += v * v
                acs += ac * ac
            v2s = np.maximum(v2s, vs)
            a2s = np.maximum(a2s, acs)
        v2 = np.maximum.reduceat(v2s, so[:-1])
        a2 = np.maximum.reduceat(a2s, so[:-1])
        ratio = np.maximum(np.sqrt(v2) / v_max, np.sqrt(np.sqrt(a2) / a_max))
        stretched = (ratio > dead_band) & (ratio < np.inf)
        factor = np.where(stretched, np.minimum(overshoot * ratio, max_stretch), 1.0)
    return T * factor[traj], np.where(stretched, np.diff(so), 0).astype(np.int32)


def peak_sites(case):
    """Where the deciding peak of every trajectory sits: (local segment, sample, share of the peak's square carried by each axis [n][3]);
    speed or acceleration, whichever sets rho.  For checking that a designed input is what it was designed to be."""
    r, so = case["r"], case["seg_offsets64"]
    nc = 2 * r
    C, traj = segment_view(r, so, case["coeff"])
    t = case["times"][:, None] * (np.arange(SAMPLES + 1) / SAMPLES)[None, :]
    by_speed = np.asarray(case["ref"]["rho_v"] >= case["ref"]["rho_a"])
    seg, smp, share = [], [], []
    for b in range(case["n_traj"]):
        sl = slice(int(so[b]), int(so[b + 1]))
        d = 1 if by_speed[b] else 2
        q = sum(np.prod(np.arange(j - d + 1, j + 1)) * C[sl, :, j, None] * t[sl, None, :] ** (j - d) for j in range(d, nc)) ** 2   # [M][3][S+1]
        tot = q.sum(axis=1)
        i, s = np.unravel_index(np.argmax(tot), tot.shape)
        seg.append(i), smp.append(s), share.append(q[i, :, s] / tot[i, s])
    return np.array(seg), np.array(smp), np.array(share)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
EPS_SHAPE = 0.05     # a planted peak falls off by 5 % along its segment: small derivatives (the other limit stays slack), and the
                     # neighbouring sample is ~2e-4 (interior) to 3e-3 (ends) lower -- far above the 1e-12 of the comparison


def _plant(c_seg_axis, kind, pos, T, amp, samples):
    """Add to one segment and axis (ascending powers) a velocity (kind 'v') or acceleration ('a') profile amp * shape(t / T) whose largest
    sample is sample 0 (pos 'first'), sample `samples` ('last') or sample pos (an int) in between."""
    e = EPS_SHAPE
    if pos == "first":
        p = np.array([1.0, -e / T, 0.0])                                  # shape(t) = p0 + p1 t + p2 t^2
    elif pos == "last":
        p = np.array([1.0 - e, e / T, 0.0])
    else:
        u = pos / samples
        p = np.array([1.0 - e * u * u, 2.0 * e * u / T, -e / (T * T)])
    p = amp * p
    if kind == "v":
        c_seg_axis[1] += p[0]
        c_seg_axis[2] += p[1] / 2.0
        c_seg_axis[3] += p[2] / 3.0
    else:
        c_seg_axis[2] += p[0] / 2.0
        c_seg_axis[3] += p[1] / 6.0
        c_seg_axis[4] += p[2] / 12.0
        c_seg_axis[1] -= amp * T / 2.0                                    # centres the velocity this acceleration integrates to


def _background(rng, r, M):
    """Small smooth coefficients on every axis and segment: |v| ~ 0.5 m/s, |a| ~ 0.5 m/s^2."""
    nc = 2 * r
    fact = np.cumprod(np.concatenate([[1.0], np.arange(1, nc)]))
    return rng.uniform(-1.0, 1.0, size=(3, M, nc)) * 0.3 / fact


def _rescale_to_targets(r, case, target):
    """Scale all coefficients of trajectory b by one number so that the reference rho becomes target[b] (NaN: leave it).  rho is linear
    in the coefficients when the speed decides and goes with their square root when the acceleration does."""
    n, uni, so = case["n_traj"], case["uniform"], case["seg_offsets64"]
    ref = reference(r, n, uni, so, case["times"], case["coeff"])
    k = np.where(ref["rho_v"] >= ref["rho_a"], target / ref["rho"], (target / ref["rho"]) ** 2).astype(np.float64)
    k = np.where(np.isnan(target), 1.0, k)
    per_coeff = np.repeat(k, 3 * 2 * r * np.diff(so))
    case["coeff"] = case["coeff"] * per_coeff


def _finish(r, case):
    so = case["seg_offsets64"]
    case["seg_offsets"] = so.astype(np.int32)
    case["M"] = np.diff(so)
    case["r"] = r
    case["ref"] = reference(r, case["n_traj"], case["uniform"], so, case["times"], case["coeff"])
    return case


def _build(r, seed, specs, uniform=0):
    """specs: one dict per trajectory -- M, cls ('plain' / 'band': stay, 'v' / 'a': stretch, 'vcap' / 'acap': hit max_stretch), and for
    the planted ones seg, axis, pos."""
    rng = np.random.default_rng(seed)
    so = np.concatenate([[0], np.cumsum([s["M"] for s in specs])]).astype(np.int64)
    times, coeff, target = [], [], []
    for s in specs:
        M = s["M"]
        T = rng.uniform(0.6, 1.4, size=M)
        T[rng.integers(0, M)] = 1.0                      # the applied factor can be read back from this segment bit for bit
        c = _background(rng, r, M)
        cls = s["cls"]
        if cls != "plain":
            kind = "a" if cls in ("a", "acap") or (cls == "band" and s["axis"] == 1) else "v"
            c[:, s["seg"], :] *= 0.1                     # (so that the background's drift does not move the peak off its designed sample)
            c[s["axis"], s["seg"], :] = 0.0
            _plant(c[s["axis"], s["seg"]], kind, s["pos"], T[s["seg"]], (V_MAX if kind == "v" else A_MAX) * 1.2, SAMPLES)
        target.append({"plain": np.nan, "band": rng.uniform(1.002, 1.008), "v": rng.uniform(1.02, 1.4), "a": rng.uniform(1.02, 1.4),
                       "vcap": rng.uniform(1.5, 1.7), "acap": rng.uniform(1.5, 1.7)}[cls])
        times.append(T)
        coeff.append(c.ravel())
    case = dict(n_traj=len(specs), uniform=uniform, seg_offsets64=so, times=np.concatenate(times), coeff=np.concatenate(coeff), specs=specs)
    _rescale_to_targets(r, case, np.array(target))
    return _finish(r, case)


def _specs_from(planted, m_of):
    """Lay the planted specs on the S slots of WAVE_PATTERN, 'plain' and 'band' trajectories alternating on the U slots."""
    specs, it, n_u = [], iter(planted), 0
    nxt = next(it, None)
    while nxt is not None:
        for slot in WAVE_PATTERN:
            b = len(specs)
            if slot == "S" and nxt is not None:
                specs.append(dict(nxt, M=m_of(b) if "M" not in nxt else nxt["M"]))
                nxt = next(it, None)
            else:
                M = m_of(b)
                specs.append(dict(M=M, cls="band" if n_u % 2 else "plain", seg=(7 * b) % M, axis=b % 3, pos=("first", 5, "last")[b % 3]))
                n_u += 1
    return specs


@functools.lru_cache(maxsize=None)
def designed_cases(r):
    """name -> case (made once per process and shared: treat it as read-only).  A case: n_traj, uniform, seg_offsets (int32), times, coeff, M, specs, ref (reference() on it)."""
    pos3 = ("first", 11, "last")
    cases = {}
    # the peak in every segment of a 17-segment trajectory (a lane's second and third pass, the last segment); uniform layout
    sweep = [dict(cls=("v", "a")[i % 2], seg=i, axis=i % 3, pos=pos3[(i // 3) % 3]) for i in range(17)]
    cases["sweep17"] = _build(r, 1700 + r, _specs_from(sweep, lambda b: 17), uniform=17)
    # first / interior / last sample x the axis that carries the peak x speed / acceleration; uniform layout, 9 segments
    grid = [dict(cls=cls, seg=(3 * k + 8 * a) % 9, axis=a, pos=pos3[k]) for cls in ("v", "a") for k in range(3) for a in range(3)]
    cases["sample_axis"] = _build(r, 900 + r, _specs_from(grid, lambda b: 9), uniform=9)
    # ragged, every M of the pool, all classes interleaved
    mix = []
    for i in range(30):
        M = M_POOL[(3 * i + 1) % len(M_POOL)]
        mix.append(dict(M=M, cls=("v", "a", "vcap", "a", "v", "acap")[i % 6], seg=(5 * i + M - 1) % M, axis=(i // 2) % 3, pos=pos3[i % 3]))
    cases["ragged_mix"] = _build(r, 6300 + r, _specs_from(mix, lambda b: M_POOL[b % len(M_POOL)]))
    return cases


@functools.lru_cache(maxsize=None)
def big_ragged_case(n_traj=65536 + 11, seed=65547):
    """Made once per process and shared: read-only.  r = 3, M in {1, 2, 3}; half of the trajectories stay (rho 0.3 .. 0.95), the others stretch (rho 1.02 .. 2: some hit max_stretch)."""
    r = 3
    rng = np.random.default_rng(seed)
    M = rng.integers(1, 4, size=n_traj)
    so = np.concatenate([[0], np.cumsum(M)]).astype(np.int64)
    tot = int(so[-1])
    T = rng.uniform(0.6, 1.4, size=tot)
    T[so[:-1] + rng.integers(0, 1 << 30, size=n_traj) % M] = 1.0
    fact = np.cumprod(np.concatenate([[1.0], np.arange(1, 2 * r)]))
    coeff = (rng.uniform(-1.0, 1.0, size=(3 * tot, 2 * r)) / fact).ravel()
    target = np.where(rng.random(n_traj) < 0.5, rng.uniform(0.3, 0.95, size=n_traj), rng.uniform(1.02, 2.0, size=n_traj))
    case = dict(n_traj=n_traj, uniform=0, seg_offsets64=so, times=T, coeff=coeff, specs=None)
    _rescale_to_targets(r, case, target)
    return _finish(r, case)
