"""Reference and inputs for the tests of the four samplers of include/uavqp.h -- uavqp_eval_batch_device, uavqp_traj_length_device,
uavqp_ellipsoid_check_device, uavqp_ellipsoid_check_grid_device: tests/test_sampler_contract.py (CPU) and tests/test_gpu_samplers.py.
Nothing here touches a GPU, and everything is restated from the header, not from the kernels.

segment_rule_scalar()   the header's segment search, one sample, written as the header states it (float64: that arithmetic IS the rule)
segment_rule()          the same for an array of samples of one trajectory, with a record of whether every step was exact
eval_reference()        position / velocity / acceleration in np.longdouble at the (segment, local time) the rule chose, and the sum S
                        of the absolute terms that the derived tolerance 32 * 2^-53 * S is made of
horner_float64()        Horner from the highest power with the factor folded into the coefficient, in numpy float64
length_reference()      sample count by the accumulated float64 loop, chords in np.longdouble at t_s = s * dt, the derived bound
ellipsoid_reference()   per-sample verdicts of the header's frame and metric in np.longdouble, first_hit derived from them
eval_cases(r) / length_case(r) / ellipsoid_cases(r) / grid_geometry_cases()    the designed inputs (made once per process: read-only)

Time grids are exact by construction: durations are multiples of 2^-6, t0 and dt dyadic with dt >= 2^-14, so t0 + s * dt and every
running t - T_i are representable and a fused multiply-add cannot move a sample across a class boundary.

Coefficient layout (include/uavqp.h): trajectory b starts at 3 * 2r * seg_offsets[b], inside it [axis][segment][2r], ascending powers.
"""
import functools

import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
SLACK = 1e-4
G = 9.81
DT14 = 2.0 ** -14
ROBOT_R, ROBOT_H = 0.4, 0.1          # the reference's launch-file robot: wide axes 0.4, thin axis 0.1; 0.4 + 0.1 == 0.5 exactly in float64
RAD = ROBOT_R + 0.1


def offsets_of(n_traj, uniform, seg_offsets):
    return np.arange(n_traj + 1, dtype=np.int64) * uniform if uniform > 0 else np.asarray(seg_offsets, dtype=np.int64)


def traj_coeff(r, so, coeff, b):
    """[3][M_b][2r] view of trajectory b."""
    nc, M = 2 * r, int(so[b + 1] - so[b])
    return np.asarray(coeff)[3 * nc * int(so[b]):3 * nc * int(so[b + 1])].reshape(3, M, nc)


# ---------------------------------------------------------------------------------------------------------------------------------
# the segment rule
# ---------------------------------------------------------------------------------------------------------------------------------
def segment_rule_scalar(T, t):
    """include/uavqp.h: walk while t > T_idx + 1e-4, subtracting; past the end clamp to the last segment's end.  float64 throughout,
    T_idx + 1e-4 rounded once.  Returns (segment, local time, clamped)."""
    T = np.asarray(T, dtype=np.float64)
    t = np.float64(t)
    idx, M = 0, T.size
    while idx < M and t > np.float64(T[idx] + np.float64(SLACK)):
        t = np.float64(t - T[idx])
        idx += 1
    if idx == M:
        return M - 1, np.float64(T[M - 1]), True
    return idx, t, False


def segment_rule(T, t):
    """The same for an array t of samples of one trajectory (M >= 1).  Returns idx, local time, clamped, and `exact`: True where every
    t - T_i taken on the way equals the longdouble difference rounded to float64 (no rounding happened at all)."""
    T = np.asarray(T, dtype=np.float64)
    t = np.array(t, dtype=np.float64)
    idx = np.zeros(t.shape, dtype=np.int64)
    going = np.ones(t.shape, dtype=bool)
    exact = np.ones(t.shape, dtype=bool)
    for i in range(T.size):
        adv = going & (t > np.float64(T[i] + np.float64(SLACK)))
        d = t - T[i]
        exact &= ~adv | ((LD(1) * t - LD(T[i])).astype(np.float64) == d) & ((LD(1) * d + LD(T[i])) == LD(1) * t)
        t = np.where(adv, d, t)
        idx += adv
        going = adv
    clamped = idx == T.size
    idx = np.where(clamped, T.size - 1, idx)
    t = np.where(clamped, T[-1], t)
    return idx, t, clamped, exact


def grid_times(n_samples, t0, dt):
    """t_s = t0 + s * dt in float64 (product rounded, then the sum) and whether the longdouble value -- what a fused multiply-add
    returns after its one rounding -- is the same double."""
    s = np.arange(n_samples, dtype=np.float64)
    t = np.float64(t0) + s * np.float64(dt)
    fused = (LD(t0) + LD(1) * s * LD(dt))
    return t, (fused.astype(np.float64) == t) & (fused == LD(1) * t)


def sample_classes(T, t_global, idx, tl, clamped):
    """Class flags of samples of one trajectory: on_knot (local time exactly the segment's duration, not clamped), in_slack (beyond the
    segment's end but within the slack: the earlier segment is evaluated past its end), advanced, clamped, negative."""
    T = np.asarray(T, dtype=np.float64)
    return dict(on_knot=~clamped & (tl == T[idx]), in_slack=~clamped & (tl > T[idx]), advanced=idx > 0, clamped=clamped, negative=t_global < 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# polynomial values
# ---------------------------------------------------------------------------------------------------------------------------------
def _falling(j, d):
    f = 1
    for q in range(d):
        f *= j - q
    return f


def poly_longdouble(C, idx, tl, derivs=(0, 1, 2)):
    """C [3][M][2r], idx / tl [n].  Returns (values LD [n][len(derivs)][3], S LD the same shape): plain power sums in longdouble,
    S = sum_j f_j |c_j| |t|^(j-d)."""
    nc = C.shape[2]
    t = LD(1) * np.asarray(tl, dtype=np.float64)
    c = C[:, idx, :].astype(LD)                                   # [3][n][nc]
    val = np.zeros((t.size, len(derivs), 3), dtype=LD)
    S = np.zeros_like(val)
    for k, d in enumerate(derivs):
        for j in range(d, nc):
            p = t ** (j - d)
            val[:, k, :] += (LD(_falling(j, d)) * c[:, :, j] * p[None, :]).T
            S[:, k, :] += (LD(_falling(j, d)) * np.abs(c[:, :, j]) * np.abs(p)[None, :]).T
    return val, S


def horner_float64(C, idx, tl, derivs=(0, 1, 2)):
    """Horner on the d-th derivative from the highest power, factor times coefficient rounded, one multiply and one add per step."""
    nc = C.shape[2]
    t = np.asarray(tl, dtype=np.float64)
    out = np.zeros((t.size, len(derivs), 3))
    for k, d in enumerate(derivs):
        for ax in range(3):
            acc = np.zeros(t.size)
            for j in range(nc - 1, d - 1, -1):
                acc = acc * t + float(_falling(j, d)) * C[ax, idx, j]
            out[:, k, ax] = acc
    return out


def eval_reference(r, n_traj, uniform, seg_offsets, times, coeff, n_samples, t0, dt):
    """What uavqp_eval_batch_device returns for what = 7, as [n_traj][n_samples][3 (pos, vel, acc)][3 (xyz)] longdouble, with S of the
    same shape, and per sample idx, local time, clamped, exact (grid and every subtraction), M per trajectory.  Zero-segment
    trajectories: zeros (S zero as well: their rows must be exactly zero)."""
    so = offsets_of(n_traj, uniform, seg_offsets)
    T_all = np.asarray(times, dtype=np.float64)
    tg, ex_grid = grid_times(n_samples, t0, dt)
    out = np.zeros((n_traj, n_samples, 3, 3), dtype=LD)
    S = np.zeros_like(out)
    idx = np.zeros((n_traj, n_samples), dtype=np.int64)
    tl = np.zeros((n_traj, n_samples))
    clamped = np.zeros((n_traj, n_samples), dtype=bool)
    exact = np.ones((n_traj, n_samples), dtype=bool)
    for b in range(n_traj):
        T = T_all[so[b]:so[b + 1]]
        if T.size == 0:
            continue
        idx[b], tl[b], clamped[b], ex = segment_rule(T, tg)
        exact[b] = ex & ex_grid
        out[b], S[b] = poly_longdouble(traj_coeff(r, so, coeff, b), idx[b], tl[b])
    return dict(out=out, S=S, idx=idx, tl=tl, clamped=clamped, exact=exact, t=tg, M=np.diff(so))


def select_what(arr, what):
    """[..., 3, 3] -> [..., K, 3] with the derivative orders of the mask `what` in pos, vel, acc order."""
    return arr[..., [d for d in range(3) if (what >> d) & 1], :]


# ---------------------------------------------------------------------------------------------------------------------------------
# length
# ---------------------------------------------------------------------------------------------------------------------------------
def count_samples(total, dt):
    """PolyTraj::getTraj's loop: t = 0; while t < total: t += dt (float64, accumulated).  Returns (count, last t)."""
    t, n, total, dt = np.float64(0.0), 0, np.float64(total), np.float64(dt)
    while t < total:
        t = np.float64(t + dt)
        n += 1
    return n, float(t)


def length_reference(r, n_traj, uniform, seg_offsets, times, coeff, dt):
    """include/uavqp.h uavqp_traj_length_device.  total = the durations added in order (float64); count by the accumulated loop;
    positions in longdouble at t_s = s * dt (the float64 product) through the segment rule; length = sum of chords; mean = length / total
    (a zero-segment trajectory: count 0, length 0, mean 0 / 0 = NaN).  bound[b]: per chord the 32 * 2^-53 * S bound on both end
    points (Euclidean norm over the axes) plus 4 * 2^-53 * chord for the differences, squares, sum and root, summed over the chords,
    plus n * 2^-53 * length for the parallel sum.  Returns dict(n, length LD, mean LD, bound LD, total)."""
    so = offsets_of(n_traj, uniform, seg_offsets)
    T_all = np.asarray(times, dtype=np.float64)
    n = np.zeros(n_traj, dtype=np.int32)
    length = np.zeros(n_traj, dtype=LD)
    bound = np.zeros(n_traj, dtype=LD)
    total = np.zeros(n_traj)
    for b in range(n_traj):
        T = T_all[so[b]:so[b + 1]]
        tot = np.float64(0.0)
        for x in T:
            tot = np.float64(tot + x)
        total[b] = tot
        n[b], _ = count_samples(tot, dt)
        if T.size == 0 or n[b] < 2:
            continue
        ts = np.arange(n[b], dtype=np.float64) * np.float64(dt)
        idx, tl, _, _ = segment_rule(T, ts)
        p, S = poly_longdouble(traj_coeff(r, so, coeff, b), idx, tl, derivs=(0,))
        p, S = p[:, 0, :], S[:, 0, :]
        chord = np.sqrt(np.sum((p[1:] - p[:-1]) ** 2, axis=1))
        ep = LD(32 * U53) * np.sqrt(np.sum(S * S, axis=1))
        length[b] = np.sum(chord)
        bound[b] = np.sum(ep[1:] + ep[:-1] + LD(4 * U53) * chord) + LD(int(n[b]) * U53) * length[b]
    with np.errstate(all="ignore"):
        mean = length / total.astype(LD)
    return dict(n=n, length=length, mean=mean, bound=bound, total=total)


# ---------------------------------------------------------------------------------------------------------------------------------
# ellipsoid check
# ---------------------------------------------------------------------------------------------------------------------------------
def frame_longdouble(acc):
    """acc LD [n][3] -> b1, b2, b3 LD [n][3]: b3 = normalize(acc + 9.81 z), b2 = normalize(b3 x (1,0,0)), b1 = normalize(b2 x b3).
    A zero vector cannot be normalised: its components become NaN and carry through (degenerate attitude)."""
    with np.errstate(all="ignore"):
        v = acc + np.array([0, 0, LD(G)], dtype=LD)[None, :]
        b3 = v / np.sqrt(np.sum(v * v, axis=1))[:, None]
        c = np.cross(b3, np.array([1, 0, 0], dtype=LD)[None, :])
        b2 = c / np.sqrt(np.sum(c * c, axis=1))[:, None]
        c = np.cross(b2, b3)
        b1 = c / np.sqrt(np.sum(c * c, axis=1))[:, None]
    return b1, b2, b3


def metric_longdouble(p, frame, obs, robot_r=ROBOT_R, robot_h=ROBOT_H):
    """|E^-1 (o - p)| for every (sample, point): LD [n][n_obs], and the distances |o - p| of the same shape."""
    b1, b2, b3 = frame
    d = LD(1) * np.asarray(obs, dtype=np.float64)[None, :, :] - p[:, None, :]
    with np.errstate(all="ignore"):
        e1 = np.einsum("nk,nok->no", b1, d) / LD(robot_r)
        e2 = np.einsum("nk,nok->no", b2, d) / LD(robot_r)
        e3 = np.einsum("nk,nok->no", b3, d) / LD(robot_h)
        return np.sqrt(e1 * e1 + e2 * e2 + e3 * e3), np.sqrt(np.sum(d * d, axis=2))


def ellipsoid_reference(r, n_traj, uniform, seg_offsets, times, coeff, n_samples, t0, dt, obs, robot_r=ROBOT_R, robot_h=ROBOT_H,
                        gravity=G, swap_axes=False):
    """Per-sample verdicts [n_traj][n_samples] uint8 and first_hit [n_traj] (n_samples: collision-free) of include/uavqp.h: a sample
    collides when a point within robot_r + 0.1 of it has |E^-1 (o - p)| <= 1.  A degenerate attitude (b3 or b2 cannot be normalised)
    and a zero-segment trajectory are collision-free.  Samples that share (trajectory, segment, local time) -- everything past the
    end -- are computed once.  Also min_margin: the smallest | metric - 1 | over all candidate pairs, and exact as in eval_reference.
    gravity / swap_axes: deliberately wrong models, for checking that a designed input tells them apart."""
    so = offsets_of(n_traj, uniform, seg_offsets)
    T_all = np.asarray(times, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3)
    tg, ex_grid = grid_times(n_samples, t0, dt)
    flags = np.zeros((n_traj, n_samples), dtype=np.uint8)
    exact = np.ones((n_traj, n_samples), dtype=bool)
    clamped = np.zeros((n_traj, n_samples), dtype=bool)
    margins, pos = [], [None] * n_traj
    rr, rh = (robot_h, robot_r) if swap_axes else (robot_r, robot_h)
    for b in range(n_traj):
        T = T_all[so[b]:so[b + 1]]
        if T.size == 0:
            continue
        idx, tl, clamped[b], ex = segment_rule(T, tg)
        exact[b] = ex & ex_grid
        key = np.stack([idx.astype(np.float64), tl], axis=1)
        uniq, inv = np.unique(key, axis=0, return_inverse=True)
        inv = np.asarray(inv).ravel()
        val, _ = poly_longdouble(traj_coeff(r, so, coeff, b), uniq[:, 0].astype(np.int64), uniq[:, 1], derivs=(0, 2))
        p, acc = val[:, 0, :], val[:, 1, :] + np.array([0, 0, LD(gravity) - LD(G)], dtype=LD)[None, :]
        hit = np.zeros(uniq.shape[0], dtype=bool)
        if obs.shape[0]:
            m, dist = metric_longdouble(p, frame_longdouble(acc), obs, rr, rh)
            with np.errstate(invalid="ignore"):
                cand = dist <= LD(robot_r) + LD(0.1)
                hit = np.any(cand & (m <= 1), axis=1)
            margins.append((np.abs(m - 1), np.abs(dist - (LD(robot_r) + LD(0.1))), inv))
        flags[b] = hit[inv]
        pos[b] = p[inv]
    first = np.where(flags.any(axis=1), flags.argmax(axis=1), n_samples).astype(np.int32)
    return dict(flags=flags, first_hit=first, exact=exact, clamped=clamped, margins=margins, pos=pos)


# ---------------------------------------------------------------------------------------------------------------------------------
# designed inputs: evaluation
# ---------------------------------------------------------------------------------------------------------------------------------
def designed_coeff(r, Ms, seed):
    """Order-1 coefficients, all distinct, random sign, magnitude 0.5 .. 1.5 divided by j! (so that the derivatives stay order 1 too):
    neighbouring segments have nothing in common."""
    rng = np.random.default_rng(seed)
    nc = 2 * r
    fact = np.cumprod(np.concatenate([[1.0], np.arange(1, nc)]))
    blocks = [(rng.uniform(0.5, 1.5, size=(3, M, nc)) * rng.choice([-1.0, 1.0], size=(3, M, nc)) / fact).ravel() for M in Ms]
    return np.concatenate(blocks) if blocks else np.zeros(0)


def designed_durations(Ms, seed):
    """Multiples of 2^-6 between 0.375 and 1.125, no two neighbours equal."""
    rng = np.random.default_rng(seed)
    out = []
    for M in Ms:
        k = rng.integers(24, 73, size=M)
        for i in range(1, M):
            if k[i] == k[i - 1]:
                k[i] += 1
        out.append(k / 64.0)
    return np.concatenate(out) if out else np.zeros(0)


def knot_time(T, k):
    """Global time of the end of segment k (exact: durations are multiples of 2^-6)."""
    return float(np.sum(T[:k + 1]))


def tight_pair(T, k):
    """The largest double t0 for which a single sample does NOT leave segment k through its end, and the next double above it (which
    does).  For k = 0 that is fl(T_0 + 1e-4) itself and its successor."""
    T = np.asarray(T, dtype=np.float64)
    base = LD(float(np.sum(T[:k]))) + LD(np.float64(T[k] + np.float64(SLACK)))
    t0 = np.float64(base)
    past = lambda t: segment_rule_scalar(T, t)[0] > k or (k == T.size - 1 and segment_rule_scalar(T, t)[2])
    while past(t0):
        t0 = np.nextafter(t0, -np.inf)
    while not past(np.nextafter(t0, np.inf)):
        t0 = np.nextafter(t0, np.inf)
    return float(t0), float(np.nextafter(t0, np.inf))


RAGGED_MS = (3, 1, 17, 0, 1, 5, 2, 17)          # M = 1 twice, a zero-segment trajectory in the middle
UNIFORM_M, UNIFORM_N = 17, 5


def _eval_grids(so, T_all, targets):
    """Windows of 32 samples at dt = 2^-14 that start 8 samples before the first, an interior and the last knot of the target
    trajectories (sample 8 on the knot, 9 inside the slack, 10 advanced or clamped), single samples on the tightest pair of doubles
    around the threshold at those knots, and one coarse grid from t < 0 to far past the longest trajectory."""
    grids = []
    for b in targets:
        T = T_all[so[b]:so[b + 1]]
        M = T.size
        for k in sorted({0, M // 2, M - 1}):
            K = knot_time(T, k)
            grids.append(dict(name=f"window-b{b}-k{k}", kind="window", b=b, k=k, n_samples=32, t0=K - 8 * DT14, dt=DT14))
            lo, hi = tight_pair(T, k)
            grids.append(dict(name=f"stay-b{b}-k{k}", kind="stay", b=b, k=k, n_samples=1, t0=lo, dt=DT14))
            grids.append(dict(name=f"leave-b{b}-k{k}", kind="leave", b=b, k=k, n_samples=1, t0=hi, dt=DT14))
    longest = max(float(np.sum(T_all[so[b]:so[b + 1]])) for b in range(so.size - 1))
    grids.append(dict(name="coarse", kind="coarse", n_samples=int((longest + 4.0) * 32) + 9, t0=-0.25, dt=2.0 ** -5))
    return grids


@functools.lru_cache(maxsize=None)
def eval_cases(r):
    """name -> case: r, n_traj, uniform, seg_offsets (int32), seg_offsets64, times, coeff, M, grids (each with its reference `ref`)."""
    cases = {}
    for name, Ms, uniform, targets in (("uniform17", (UNIFORM_M,) * UNIFORM_N, UNIFORM_M, (0, 4)), ("ragged", RAGGED_MS, 0, (0, 1, 2, 4, 7))):
        so = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int64)
        case = dict(r=r, n_traj=len(Ms), uniform=uniform, seg_offsets64=so, seg_offsets=so.astype(np.int32), M=np.asarray(Ms),
                    times=designed_durations(Ms, 100 * r + len(Ms)), coeff=designed_coeff(r, Ms, 1000 * r + len(Ms)))
        case["grids"] = _eval_grids(so, case["times"], targets)
        for g in case["grids"]:
            g["ref"] = eval_reference(r, case["n_traj"], uniform, so, case["times"], case["coeff"], g["n_samples"], g["t0"], g["dt"])
        cases[name] = case
    return cases


# ---------------------------------------------------------------------------------------------------------------------------------
# designed inputs: length
# ---------------------------------------------------------------------------------------------------------------------------------
LENGTH_DT = 2.0 ** -6
# total time in 1/64 s -> samples at dt = 2^-6: 1 (dt exceeds the total time), 2, 64, 65, 129; the wave's stride loop over the chords
# runs 0, 1 and several rounds; 0 segments in the middle
LENGTH_MS = (1, 1, 1, 0, 2, 3, 1)
LENGTH_TOTALS64 = ((1,), (2,), (64,), (), (40, 25), (50, 40, 39), (32,))
# the reference's own sampling: dt = 0.01, 1.0 s per segment.  M -> the accumulated t after 100 M additions is >= M (100 M samples) or
# still below it (one sample more); found on the CPU, pinned in tests/test_sampler_contract.py
ACCUMULATION_MS = (1, 2, 3, 4, 5, 6, 7)


def _line_coeff(r, T, p0, v):
    """One straight line through all segments: c0 = p0 + v K_i, c1 = v."""
    M, nc = T.size, 2 * r
    c = np.zeros((3, M, nc))
    K = np.concatenate([[0.0], np.cumsum(T)[:-1]])
    c[:, :, 0] = p0[:, None] + v[:, None] * K[None, :]
    c[:, :, 1] = v[:, None]
    return c.ravel()


@functools.lru_cache(maxsize=None)
def length_cases(r):
    """'dyadic': ragged, dt = 2^-6, discontinuous designed polynomials; 'line': the same batch with one straight line per trajectory
    (length = |v| (n - 1) dt in closed form); 'accumulated': uniform-free batch of M x 1.0 s trajectories at the reference's dt = 0.01."""
    cases = {}
    so = np.concatenate([[0], np.cumsum(LENGTH_MS)]).astype(np.int64)
    T = np.array([x / 64.0 for tot in LENGTH_TOTALS64 for x in tot])
    rng = np.random.default_rng(77 + r)
    v = rng.uniform(-2.0, 2.0, size=(len(LENGTH_MS), 3))
    p0 = rng.uniform(-5.0, 5.0, size=(len(LENGTH_MS), 3))
    line = np.concatenate([_line_coeff(r, T[so[b]:so[b + 1]], p0[b], v[b]) for b in range(len(LENGTH_MS))])
    for name, coeff in (("dyadic", designed_coeff(r, LENGTH_MS, 500 + r)), ("line", line)):
        cases[name] = dict(r=r, n_traj=len(LENGTH_MS), uniform=0, seg_offsets64=so, seg_offsets=so.astype(np.int32), times=T, coeff=coeff,
                           dt=LENGTH_DT, v=v)
    so = np.concatenate([[0], np.cumsum(ACCUMULATION_MS)]).astype(np.int64)
    cases["accumulated"] = dict(r=r, n_traj=len(ACCUMULATION_MS), uniform=0, seg_offsets64=so, seg_offsets=so.astype(np.int32),
                                times=np.ones(int(so[-1])), coeff=designed_coeff(r, ACCUMULATION_MS, 600 + r), dt=0.01)
    # the length kernel's own copy of the segment rule: at dt = 2^-14 sample 512 is on the knot of a (2/64, 1/64) s trajectory, 513 inside the
    # slack (the first segment, past its end), 514 in the second; with dt = fl(0.5 + 1e-4) sample 1 IS the threshold of a (0.5, 0.5) s one
    for name, T2, dt in (("slack", (2.0 / 64, 1.0 / 64), DT14), ("threshold", (0.5, 0.5), float(np.float64(0.5 + SLACK)))):
        so = np.array([0, 2], dtype=np.int64)
        cases[name] = dict(r=r, n_traj=1, uniform=2, seg_offsets64=so, seg_offsets=so.astype(np.int32), times=np.array(T2),
                           coeff=designed_coeff(r, (2,), 700 + r), dt=dt)
    for c in cases.values():
        c["ref"] = length_reference(r, c["n_traj"], 0, c["seg_offsets64"], c["times"], c["coeff"], c["dt"])
    return cases


# ---------------------------------------------------------------------------------------------------------------------------------
# designed inputs: ellipsoid check
# ---------------------------------------------------------------------------------------------------------------------------------
# attitudes by the acceleration of a segment (its c2 is half of it): hover, tilted about y, about x, both, and a strong one
ATTITUDES = ((0.0, 0.0, 0.0), (6.0, 0.0, 0.0), (0.0, 6.0, 0.0), (3.0, -4.0, 2.0), (-8.0, 5.0, -3.0))
# unit directions in the BODY frame (b1, b2, b3): the three axes and two diagonals
BODY_DIRS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (2.0 / 3.0, -2.0 / 3.0, 1.0 / 3.0))
EPS_SURFACE = 1e-6


def moving_coeff(r, Ms, seed, speed=4.0, vertical=False):
    """Segments that have nothing in common: start positions on a 6 m lattice (z between 2 and 4), a velocity of `speed` m/s (neighbouring
    samples at dt = 2^-2 are 1 m apart: a point on one sample's ellipsoid is no candidate of another), the acceleration cycling through
    ATTITUDES, small distinct higher coefficients."""
    rng = np.random.default_rng(seed)
    nc = 2 * r
    blocks, spot = [], 0
    for M in Ms:
        c = np.zeros((3, M, nc))
        for i in range(M):
            c[:, i, 0] = (6.0 * (spot % 5), 6.0 * (spot // 5 % 5), 2.0 + 0.25 * (spot % 9))
            d = np.array([0.0, 0.0, 1.0]) if vertical else np.array([np.cos(0.7 * spot), np.sin(0.7 * spot), 0.05])
            c[:, i, 1] = speed * d / np.linalg.norm(d)
            c[:, i, 2] = 0.5 * np.array(ATTITUDES[spot % len(ATTITUDES)])
            c[:, i, 3:] = rng.uniform(0.01, 0.03, size=(3, nc - 3)) * rng.choice([-1.0, 1.0], size=(3, nc - 3))
            spot += 1
        blocks.append(c.ravel())
    return np.concatenate(blocks) if blocks else np.zeros(0)


def surface_point(r, case, b, s, u_body, scale):
    """p + Rot diag(robot_r, robot_r, robot_h) u * scale for sample s of trajectory b (longdouble p and frame from the reference), as
    float64 coordinates."""
    so = case["seg_offsets64"]
    T = case["times"][so[b]:so[b + 1]]
    tg, _ = grid_times(case["n_samples"], case["t0"], case["dt"])
    idx, tl, _, _ = segment_rule(T, tg[s:s + 1])
    val, _ = poly_longdouble(traj_coeff(r, so, case["coeff"], b), idx, tl, derivs=(0, 2))
    b1, b2, b3 = frame_longdouble(val[:, 1, :])
    u = np.array(u_body, dtype=LD)
    u = u / np.sqrt(np.sum(u * u))
    o = val[0, 0, :] + LD(scale) * (LD(ROBOT_R) * u[0] * b1[0] + LD(ROBOT_R) * u[1] * b2[0] + LD(ROBOT_H) * u[2] * b3[0])
    return o.astype(np.float64)


def filler_points(n, z=-3.0):
    """n distinct points on a 0.75 m lattice in the plane z = -3: more than 5 m below every sample of the designed trajectories."""
    i = np.arange(n)
    return np.stack([-2.0 + 0.75 * (i % 40), -2.0 + 0.75 * (i // 40), np.full(n, z)], axis=1)


def _ell_case(r, name, Ms, uniform, n_samples, t0, dt, plants, n_obs, slots, seed, T=None, vertical=False, extra=None):
    """plants: (trajectory, sample, body direction, inside?) -- one decisive point each, at surface * (1 -/+ 1e-6); slots: their indices in
    the cloud (filler elsewhere)."""
    so = np.concatenate([[0], np.cumsum(Ms)]).astype(np.int64)
    case = dict(r=r, name=name, n_traj=len(Ms), uniform=uniform, seg_offsets64=so, seg_offsets=so.astype(np.int32), M=np.asarray(Ms),
                times=designed_durations(Ms, seed) if T is None else np.asarray(T, dtype=np.float64), coeff=moving_coeff(r, Ms, seed + 1, vertical=vertical),
                n_samples=n_samples, t0=t0, dt=dt, plants=plants, slots=list(slots))
    obs = filler_points(n_obs)
    assert len(plants) == len(slots) <= n_obs
    for (b, s, u, inside), slot in zip(plants, slots):
        obs[slot] = surface_point(r, case, b, s, u, 1.0 - EPS_SURFACE if inside else 1.0 + EPS_SURFACE)
    if extra is not None:
        obs = np.concatenate([obs, extra])
    case["obs"] = obs
    case["ref"] = ellipsoid_reference(r, case["n_traj"], uniform, so, case["times"], case["coeff"], n_samples, t0, dt, obs)
    return case


@functools.lru_cache(maxsize=None)
def ellipsoid_cases(r):
    """name -> case (+ n_samples, t0, dt, obs, plants, slots, ref).  dt = 2^-2, t0 = 2^-3: a sample every metre of path."""
    Q = 0.25
    cases = {}
    # every body direction, inside and outside, on every attitude; uniform, 5 segments of 1 s; n_obs = 2500 with the decisive points at
    # 0, 1023, 1024 and the last index among them; collisions at the first sample, interior ones, the last one
    U5 = (5,) * 4
    T5 = np.ones(20)
    n_s = 20                                                  # t = 0.125 .. 4.875: four samples per segment, all inside the trajectory
    plants = []
    for b in range(4):
        for i, u in enumerate(BODY_DIRS):
            s = 4 * i + (b + i) % 4                           # one sample in every segment (= every attitude)
            plants.append((b, s, u, (b + i) % 2 == 0))
    plants[0] = (0, 0, BODY_DIRS[0], True)                    # a collision at the very first sample
    plants[-1] = (3, n_s - 1, BODY_DIRS[4], True)             # and one at the very last
    slots = list(range(5, 5 + len(plants)))
    for k, slot in zip((0, 2, 4, 6), (0, 1023, 1024, 2499)):      # four INSIDE points at the first index, on both sides of the tile boundary and last
        assert plants[k][3]
        slots[k] = slot
    cases["directions"] = _ell_case(r, "directions", U5, 5, n_s, 0.125, Q, plants, 2500, slots, 40 + r, T=T5)
    # the tile loop of the exhaustive kernel: 1024 points per tile; the only decisive point at the last index
    for n_obs in (1, 1024, 1025):
        cases[f"tile{n_obs}"] = _ell_case(r, f"tile{n_obs}", (2, 3), 0, 12, 0.125, Q, [(1, 5, BODY_DIRS[3], True)], n_obs, [n_obs - 1], 50 + r)
    # ragged, with M = 1 and a zero-segment trajectory; collisions only past the end for trajectory 4 (the end point); none for 0
    Ms = (3, 1, 0, 2, 1, 4)
    plants = [(1, 2, BODY_DIRS[2], True), (3, 0, BODY_DIRS[1], False), (3, 3, BODY_DIRS[0], True), (4, 23, BODY_DIRS[4], True), (5, 9, BODY_DIRS[3], True),
              (5, 10, BODY_DIRS[2], False)]
    cases["ragged"] = _ell_case(r, "ragged", Ms, 0, 24, 0.125, Q, plants, 40, [0, 39, 7, 8, 20, 21], 60 + r)
    # more than 256 samples per trajectory: hits in the second and the third block of 256 (and two in one wave)
    plants = [(0, 300, BODY_DIRS[0], True), (0, 301, BODY_DIRS[1], True), (0, 520, BODY_DIRS[2], True), (1, 258, BODY_DIRS[3], False),
              (1, 259, BODY_DIRS[4], True)]
    cases["blocks"] = _ell_case(r, "blocks", (9, 9), 9, 600, 0.0, 2.0 ** -6, plants, 8, [0, 1, 2, 3, 4], 70 + r, T=np.full(18, 1.125))
    return cases


@functools.lru_cache(maxsize=None)
def endpoint_case(r):
    """Three trajectories of 32 samples (t0 = 2^-5, dt = 2^-4) that collide at their END POINT only; the first sample past the end is
    sample 0 (lane 0 of its wave), sample 31 of trajectory 1 (lane 63) and sample 1 of trajectory 2 (lane 1 of the second wave).
    Vertical flight at 8 m/s, the point 5 cm above the end point: the sample before the end is 0.25 m lower (metric > 1.4)."""
    Ms = (1, 2, 1)
    T = np.array([1.0 / 64, 1.0, 60.0 / 64, 3.0 / 64])
    so = np.array([0, 1, 3, 4], dtype=np.int64)
    case = dict(r=r, name="endpoint", n_traj=3, uniform=0, seg_offsets64=so, seg_offsets=so.astype(np.int32), M=np.asarray(Ms), times=T,
                coeff=moving_coeff(r, Ms, 80 + r, speed=8.0, vertical=True), n_samples=32, t0=2.0 ** -5, dt=2.0 ** -4)
    obs = filler_points(12)
    for b in range(3):
        obs[4 * b] = surface_point(r, case, b, 31, (0.0, 0.0, 1.0), 0.5)
    case["obs"] = obs
    case["ref"] = ellipsoid_reference(r, 3, 0, so, T, case["coeff"], 32, case["t0"], case["dt"], obs)
    return case


@functools.lru_cache(maxsize=None)
def knot_cases(r):
    """The check kernels' own copies of the segment rule.  One two-segment trajectory whose segments lie 6 m apart, one obstacle point half
    way inside the ellipsoid of the FIRST segment's polynomial just past its end.  'knot_window': 32 samples at dt = 2^-14 from 8 samples
    before the knot -- on the knot and inside the slack the first segment still holds (hit), from sample 10 on the second (free).
    'knot_threshold' / 'knot_above': one sample at t0 = fl(T_0 + 1e-4) (stays: hit) and at the next double (advances: free)."""
    T = np.array([48.0 / 64, 40.0 / 64])
    so = np.array([0, 2], dtype=np.int64)
    lo, hi = tight_pair(T, 0)
    cases = {}
    for name, ns, t0 in (("knot_window", 32, float(T[0]) - 8 * DT14), ("knot_threshold", 1, lo), ("knot_above", 1, hi)):
        case = dict(r=r, name=name, n_traj=1, uniform=2, seg_offsets64=so, seg_offsets=so.astype(np.int32), M=np.array([2]), times=T,
                    coeff=moving_coeff(r, (2,), 95 + r), n_samples=ns, t0=t0, dt=DT14)
        window = dict(case, n_samples=32, t0=float(T[0]) - 8 * DT14)
        obs = filler_points(5)
        obs[3] = surface_point(r, window, 0, 9, (0.6, 0.0, 0.8), 0.5)
        case["obs"] = obs
        case["ref"] = ellipsoid_reference(r, 1, 2, so, T, case["coeff"], ns, t0, DT14, obs)
        cases[name] = case
    return cases


@functools.lru_cache(maxsize=None)
def endpoint_lane0_case(r):
    """Two trajectories of 48 samples on the same grid.  Trajectory 1 (samples 48 .. 95 of the batch) lasts 1.0 s and collides at its end
    point only: its first sample past the end is s = 16, the 64th sample of the batch -- lane 0 of the second wave, with s > 0 and the
    sample before it (lane 63 of the first wave) not past the end.  Trajectory 0 lasts 3.5 s, longer than the grid, and meets nothing."""
    Ms = (1, 1)
    T = np.array([3.5, 1.0])
    so = np.array([0, 1, 2], dtype=np.int64)
    case = dict(r=r, name="endpoint_lane0", n_traj=2, uniform=1, seg_offsets64=so, seg_offsets=so.astype(np.int32), M=np.asarray(Ms), times=T,
                coeff=moving_coeff(r, Ms, 90 + r, speed=8.0, vertical=True), n_samples=48, t0=2.0 ** -5, dt=2.0 ** -4)
    obs = filler_points(6)
    obs[2] = surface_point(r, case, 1, 47, (0.0, 0.0, 1.0), 0.5)
    case["obs"] = obs
    case["ref"] = ellipsoid_reference(r, 2, 1, so, T, case["coeff"], 48, case["t0"], case["dt"], obs)
    return case


@functools.lru_cache(maxsize=None)
def beyond_grid_case(r, cus):
    """More samples than one launch of either check holds on a device of `cus` compute units (16 * cus blocks of 256 samples; the grid
    entry: 64 * cus waves of 64), an 8-point cloud.  Two short trajectories on the grid t0 = 2^-3, dt = 2^-2: the first collides at its
    END POINT only -- every past-the-end sample is a hit, in the strided rounds too, and first_hit is the first of them --, the second
    at one interior sample."""
    ns = (256 * 16 * cus) // 2 + 131
    case = dict(ellipsoid_cases(r)["tile1"])
    case.update(name="beyond", n_samples=ns, t0=0.125, dt=0.25, plants=[(1, 5, BODY_DIRS[3], True)], slots=[6])
    obs = filler_points(8)
    obs[3] = surface_point(r, case, 0, ns - 1, (0.0, 0.0, 1.0), 0.5)
    obs[6] = surface_point(r, case, 1, 5, BODY_DIRS[3], 1.0 - EPS_SURFACE)
    case["obs"] = obs
    case["ref"] = ellipsoid_reference(r, 2, 0, case["seg_offsets64"], case["times"], case["coeff"], ns, case["t0"], case["dt"], obs)
    return case


@functools.lru_cache(maxsize=None)
def degenerate_case(r):
    """Sample 0 at local time 0 of a one-segment trajectory whose acceleration there is exactly (0, 0, -9.81) (no thrust: b3 cannot be
    normalised), (3, 0, -9.81) (b3 parallel to x: b2 cannot be) and, for comparison, (3, 1e-3, -9.81) (regular).  One obstacle point
    sits ON each sample position."""
    nc = 2 * r
    acc = ((0.0, 0.0, -G), (3.0, 0.0, -G), (3.0, 1e-3, -G))
    c = np.zeros((3, 3, 1, nc))                                   # [traj][axis][segment][power]
    for b in range(3):
        c[b, :, 0, 0] = (5.0 * b, 1.0, 2.0)
        c[b, :, 0, 2] = 0.5 * np.array(acc[b])
    so = np.array([0, 1, 2, 3], dtype=np.int64)
    case = dict(r=r, name="degenerate", n_traj=3, uniform=1, seg_offsets64=so, seg_offsets=so.astype(np.int32), M=np.ones(3, dtype=int),
                times=np.ones(3), coeff=c.ravel(), n_samples=1, t0=0.0, dt=0.25, obs=np.array([[0.0, 1.0, 2.0], [5.0, 1.0, 2.0], [10.0, 1.0, 2.0]]))
    case["ref"] = ellipsoid_reference(r, 3, 1, so, case["times"], case["coeff"], 1, 0.0, 0.25, case["obs"])
    return case


# ---------------------------------------------------------------------------------------------------------------------------------
# designed geometry for the grid check: hover attitude (c2 = 0), one-segment trajectories standing still at local time 0
# ---------------------------------------------------------------------------------------------------------------------------------
def _standing(r, positions, n_samples=1):
    """One-segment trajectories (T = 1) that stand still at the given positions: hover attitude (b1, b2, b3 = x, y, z), so the ellipsoid
    is 0.4 x 0.4 x 0.1 along x, y, z."""
    nc = 2 * r
    P = np.asarray(positions, dtype=np.float64)
    c = np.zeros((P.shape[0], 3, 1, nc))
    c[:, :, 0, 0] = P
    so = np.arange(P.shape[0] + 1, dtype=np.int64)
    return dict(r=r, n_traj=P.shape[0], uniform=1, seg_offsets64=so, seg_offsets=so.astype(np.int32), M=np.ones(P.shape[0], dtype=int),
                times=np.ones(P.shape[0]), coeff=c.ravel(), n_samples=n_samples, t0=0.0, dt=0.25)


def _with_ref(case, obs):
    case["obs"] = np.asarray(obs, dtype=np.float64)
    case["ref"] = ellipsoid_reference(case["r"], case["n_traj"], case["uniform"], case["seg_offsets64"], case["times"], case["coeff"],
                                      case["n_samples"], case["t0"], case["dt"], case["obs"])
    return case


@functools.lru_cache(maxsize=None)
def grid_geometry_cases(r=3):
    """'neighbours': 26 samples, each 1 cm inside a corner / edge / face of its own 0.5 m cell, its only point 1 cm across in the
    neighbour cell (dx, dy, dz); the lattice of cells starts at the cloud's lower corner (-4, -4, -4), cell 0.5: exact boundaries.
    'bbox': samples outside the cloud's bounding box by 0.3 m along x (collides: 0.3 < 0.4) and by 0.6 m (beyond the search radius), on
    both sides, and above it by 0.09 m (collides: the thin axis is 0.1) and by 0.2 m.
    'pooled': a wave of 64 samples without a single candidate except lane 37, which has 150 -- all outside the ellipsoid but one, and
    the one is last in its cell.  'pooled_miss': the same with the decisive point 1e-6 outside."""
    cases = {}
    corner = np.array([[-4.0, -4.0, -4.0], [40.0, 8.0, 8.0]])                # fixes the bounding box: origin -4, whole cells of 0.5
    pos, pts, e = [], [], 0.01
    offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
    for k, o in enumerate(offs):
        lo = np.array([1.5 * k, 0.0, 0.0])                                    # the sample's cell [lo, lo + 0.5)
        p = lo + 0.25 + np.array(o) * (0.25 - e)                              # 1 cm inside the side(s) facing the neighbour
        q = p + np.array(o) * 2 * e                                           # 1 cm across
        pos.append(p), pts.append(q)
    cases["neighbours"] = _with_ref(_standing(r, pos), np.concatenate([corner, np.array(pts)]))
    box = np.array([[0.0, 0.0, 0.0], [4.0, 4.0, 4.0], [0.0, 2.0, 2.0], [4.0, 2.0, 2.0], [2.0, 2.0, 4.0]])
    cases["bbox"] = _with_ref(_standing(r, [[-0.3, 2.0, 2.0], [-0.6, 2.0, 2.0], [4.3, 2.0, 2.0], [4.6, 2.0, 2.0], [2.0, 2.0, 4.09], [2.0, 2.0, 4.2]]), box)
    for name, scale in (("pooled", 1.0 - EPS_SURFACE), ("pooled_miss", 1.0 + EPS_SURFACE)):
        P = np.array([[1.0 + 1.5 * (i % 16), 1.0 + 1.5 * (i // 16), 6.0] for i in range(64)])
        c = _standing(r, P)
        busy = P[37]
        rng = np.random.default_rng(37)
        d = rng.normal(size=(150, 3))
        d[:, 2] = np.abs(d[:, 2]) * 0.2
        ring = busy + d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.42, 0.49, size=150)[:, None]
        u = np.array([0.6, 0.0, 0.8])
        decisive = busy + scale * np.array([ROBOT_R * u[0], 0.0, ROBOT_H * u[2]])
        cases[name] = _with_ref(c, np.concatenate([corner, ring, decisive[None, :]]))
    return cases
