"""-m gpu: the certified bounds (uavqp_envelope_device / _host) and their facades, against the numpy reference of
tests/envelope_reference.py and the exact extrema of tests/golden/envelope_exact.json.

Tolerances (derived, not measured).  Device and reference do the same convex combinations in float64 and differ in contraction and in
the order of a sum only; the method bounds that rounding by the guard of the quantity, so every output agrees within its guard: G for an
axis range, Gq for w, and for a rooted norm Gq carried through the root, Gq / (2 value) (sqrt(Gq) at value 0).  Verdict words are equal
wherever the limits lie at least two guards from both bounds they are compared with, which the test checks on the reference.  Soundness
against the exact extrema has no tolerance on the outer pair (envelope_reference.sandwich_failures).

Shapes.  The recorded cases (r = 3 / 4; 1, 3 and 9 segments; ragged with an empty trajectory; three closed forms) at depth 0, 3, 4 and 8
(below, at and above the three splits the lanes of a group share out; the deepest); a uniform batch of 70 trajectories (past one wave of
groups); and one call on 8 x 32 x CUs + 11 trajectories, which takes the grid-stride loop a second time."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import envelope_reference as E
import uav_motion_planning_amd as U
from uav_motion_planning_amd import _lib
from uav_motion_planning_amd import workloads as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("range", "norm", "peak", "seg_verdict", "verdict")
DEPTHS = (0, 3, 4, 8)


@pytest.fixture(scope="module")
def golden():
    return E.load_golden()


def dev():
    import torch
    return torch, torch.device("cuda", 0)


def up(x):
    torch, d = dev()
    return torch.from_numpy(np.ascontiguousarray(x)).to(d)


def device_call(ctx, r, so, T, coeff, uniform=0, status=None, box=None, want=OUT, **params):
    """uavqp_envelope_device on fresh device buffers pre-filled with NaN / -1 -> dict of numpy arrays"""
    torch, d = dev()
    so = np.ascontiguousarray(so, dtype=np.int32)
    n, tot = so.size - 1, int(so[-1])
    shapes = dict(range=(tot, 4, 3, 4), norm=(tot, 5, 4), peak=(n, 5, 4), seg_verdict=(tot,), verdict=(n,))
    bufs = {k: (torch.full(shapes[k], -1, dtype=torch.int32, device=d) if "verdict" in k
                else torch.full(shapes[k], float("nan"), dtype=torch.float64, device=d)) if k in want else None for k in OUT}
    d_so, d_T, d_c = up(so), up(np.asarray(T, dtype=np.float64)), up(np.asarray(coeff, dtype=np.float64))
    d_st = None if status is None else up(np.asarray(status, dtype=np.int32))
    d_lo, d_hi = (None, None) if box is None else (up(box[0]), up(box[1]))
    torch.cuda.synchronize()
    ctx.envelope_device(r, n, uniform, None if uniform else d_so, d_T, d_c, status=d_st, box_lo=d_lo, box_hi=d_hi, range_out=bufs["range"],
                        norm_out=bufs["norm"], peak_out=bufs["peak"], seg_verdict_out=bufs["seg_verdict"], verdict_out=bufs["verdict"], **params)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items() if v is not None}


def run(ctx, c, **kw):
    return device_call(ctx, c["r"], c["seg_offsets"], c["times"], c["coeff"], **kw)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_parity(got, ref, tag):
    """every output within the guard of its quantity; the peaks are exactly the min / max of the device's own norms"""
    err = np.abs(got["range"] - ref["range"])
    assert np.array_equal(np.isnan(got["range"]), np.isnan(ref["range"])), tag
    assert np.all((err <= ref["G"][..., None]) | np.isnan(ref["range"])), (tag, float(np.nanmax(err - ref["G"][..., None])))
    assert np.array_equal(np.isnan(got["norm"]), np.isnan(ref["norm"])), tag
    with np.errstate(all="ignore"):
        tol = np.where(ref["norm"][:, :4] > 0, ref["Gq"][:, :4, None] / (2 * ref["norm"][:, :4]), np.sqrt(ref["Gq"][:, :4, None]))
    tol = np.concatenate([tol, np.broadcast_to(ref["Gq"][:, 4:, None], (tol.shape[0], 1, 4))], axis=1)
    err = np.abs(got["norm"] - ref["norm"])
    assert np.all((err <= tol) | np.isnan(ref["norm"])), (tag, float(np.nanmax(err - tol)))
    worst = float(np.nanmax(np.concatenate([(np.abs(got["range"] - ref["range"]) / np.where(ref["G"] > 0, ref["G"], np.inf)[..., None]).ravel(),
                                            (err / np.where(tol > 0, tol, np.inf)).ravel()])))
    so = ref["so"]
    for b in range(so.size - 1):
        nm = got["norm"][int(so[b]):int(so[b + 1])]
        if nm.shape[0] == 0 or not nm.any():
            continue
        want = np.concatenate([nm[:, :, :2].min(axis=0), nm[:, :, 2:].max(axis=0)], axis=1)
        assert np.array_equal(got["peak"][b], want, equal_nan=True), (tag, b)
    return worst


def reference(c, **kw):
    ref = E.envelope(c["r"], c["seg_offsets"], c["times"], c["coeff"], **kw)
    ref["so"] = np.asarray(c["seg_offsets"])
    return ref


@pytest.mark.parametrize("depth", DEPTHS)
def test_parity_and_soundness_on_the_recorded_cases(gpu_ctx, golden, depth):
    worst, bad = 0.0, []
    for name, c in golden.items():
        got = run(gpu_ctx, c, depth=depth, tilt_max=E.TILT_GOLDEN)
        assert not np.any(got["seg_verdict"] == -1) and not np.any(got["verdict"] == -1), "every element is written"
        assert not np.isnan(got["range"]).any() and not np.isnan(got["norm"]).any() and not np.isnan(got["peak"]).any(), name
        ref = reference(c, depth=depth, tilt_max=E.TILT_GOLDEN)
        worst = max(worst, assert_parity(got, ref, (name, depth)))
        bad += E.sandwich_failures(dict(got, G=ref["G"], Gq=ref["Gq"]), c["exact"], name)
    print(f"depth {depth}: worst |device - reference| = {worst:.3g} of the guard")
    assert not bad, "\n".join(bad[:20])


def limits_of(c, factor):
    """limits at `factor` x the exact peak over the whole case, a box at the exact position range moved by a tenth of its extent"""
    n = len(c["times"])
    pk = [max(float(c["exact"]["norm"][i][k][1]) for i in range(n)) for k in range(4)]
    pos = np.array([[[float(x) for x in c["exact"]["range"][i][0][ax]] for ax in range(3)] for i in range(n)])
    ext, s = pos[..., 1] - pos[..., 0], (factor - 1.0)
    lim = dict(v_max=factor * pk[0], a_max=factor * pk[1], j_max=factor * pk[2], f_max=factor * pk[3], tilt_max=E.TILT_GOLDEN)
    if factor > 1:
        lim["f_min"] = 0.5 * min(float(c["exact"]["norm"][i][3][0]) for i in range(n))
    return lim, (pos[..., 0] - s * ext, pos[..., 1] + s * ext)


def limits_are_two_guards_away(ref, lim, box):
    """the precondition of verdict parity: every comparison of the verdict is decided by more than two guards on the reference"""
    ok = True
    for k, name in enumerate(("v_max", "a_max", "j_max")):
        if lim.get(name, 0.0) > 0:
            ok &= bool(np.all(np.abs(ref["sq"][:, k, 2:] - lim[name] ** 2) > 2 * ref["Gq"][:, k, None]))
    for name, cols in (("f_min", slice(0, 2)), ("f_max", slice(2, 4))):
        if lim.get(name, 0.0) > 0:
            ok &= bool(np.all(np.abs(ref["sq"][:, 3, cols] - lim[name] ** 2) > 2 * ref["Gq"][:, 3, None]))
    if lim.get("tilt_max", 0.0) > 0:
        ok &= bool(np.all(np.abs(ref["sq"][:, 4, :2]) > 2 * ref["Gq"][:, 4, None]))
        ok &= bool(np.all(np.abs(ref["range"][:, 2, 2, :2] + E.GRAVITY) > 2 * ref["G"][:, 2, 2, None]))
    lo, hi = box
    ok &= bool(np.all(np.abs(ref["range"][:, 0, :, :2] - lo[..., None]) > 2 * ref["G"][:, 0, :, None]))
    ok &= bool(np.all(np.abs(ref["range"][:, 0, :, 2:] - hi[..., None]) > 2 * ref["G"][:, 0, :, None]))
    return ok


@pytest.mark.parametrize("depth", DEPTHS)
def test_verdict_words_equal_the_reference(gpu_ctx, golden, depth):
    compared, states = 0, set()
    for name, c in golden.items():
        for factor in (1.1, 0.9):
            lim, box = limits_of(c, factor)
            ref = reference(c, depth=depth, box_lo=box[0], box_hi=box[1], **lim)
            if not limits_are_two_guards_away(ref, lim, box):
                continue   # (the closed forms: a constant quantity sits ON the limit's side of its own peak only by the factor; a zero stays zero)
            got = run(gpu_ctx, c, depth=depth, box=box, **lim)
            assert np.array_equal(got["seg_verdict"], ref["seg_verdict"]) and np.array_equal(got["verdict"], ref["verdict"]), (name, factor)
            compared += 1
            states |= {E.decode(w, t) for w in got["verdict"] for t in E.TESTS}
    assert compared >= 16 and states == {"certified", "violated", "undecided"}


def test_closed_forms_on_the_device(gpu_ctx, golden):
    for r in (3, 4):
        ff = run(gpu_ctx, golden[f"r{r}-free_fall"], depth=4, f_min=3.0)
        assert ff["norm"][0, 3, 0] == 0.0 and E.decode(ff["verdict"][0], "f_min") == "violated"
        c = golden[f"r{r}-parabola"]
        d0 = run(gpu_ctx, c, depth=0)
        peak = float(c["exact"]["norm"][0][0][1])
        for v_max in (0.5 * (d0["norm"][0, 0, 2] + peak), 0.5 * (peak + d0["norm"][0, 0, 3])):
            assert E.decode(run(gpu_ctx, c, depth=0, v_max=v_max)["verdict"][0], "v_max") == "undecided"
            assert E.decode(run(gpu_ctx, c, depth=6, v_max=v_max)["verdict"][0], "v_max") == ("violated" if v_max < peak else "certified")


def pool_of(golden, r):
    """every recorded segment of order r as a one-segment trajectory: (T [n], coeff [n][3][2r])"""
    T = np.concatenate([c["times"] for c in golden.values() if c["r"] == r])
    C = np.concatenate([E.segment_coefficients(r, c["seg_offsets"], c["coeff"]) for c in golden.values() if c["r"] == r])
    return T, C


@pytest.mark.parametrize("r", [3, 4])
def test_uniform_batch_of_70_trajectories(gpu_ctx, golden, r):
    """70 trajectories of 2 segments (uniform, no offsets): 70 groups are past the 64 lanes of one wave and the 8 groups of one block"""
    T, C = pool_of(golden, r)
    idx = np.arange(140) % T.size
    Tb = T[idx]
    coeff = C[idx].reshape(70, 2, 3, 2 * r).transpose(0, 2, 1, 3).ravel()
    so = np.arange(71, dtype=np.int32) * 2
    st = np.full(70, U.UAVQP_SOLVED, dtype=np.int32)
    st[[3, 64]] = 2
    got = device_call(gpu_ctx, r, so, Tb, coeff, uniform=2, status=st, depth=4, v_max=3.0, a_max=6.0, tilt_max=E.TILT_GOLDEN)
    ref = E.envelope(r, so, Tb, coeff, status=st, depth=4, v_max=3.0, a_max=6.0, tilt_max=E.TILT_GOLDEN)
    ref["so"] = so
    assert_parity(got, ref, ("uniform70", r))
    for b in (3, 64):
        assert not got["range"][2 * b:2 * b + 2].any() and not got["norm"][2 * b:2 * b + 2].any() and not got["peak"][b].any()
        assert not got["seg_verdict"][2 * b:2 * b + 2].any() and got["verdict"][b] == 0
    ragged = device_call(gpu_ctx, r, so, Tb, coeff, uniform=0, status=st, depth=4, v_max=3.0, a_max=6.0, tilt_max=E.TILT_GOLDEN)
    for k in OUT:
        assert same_bytes(got[k], ragged[k]), k


def test_grid_stride_gives_the_bytes_of_a_small_call(gpu_ctx, golden):
    """8 x 32 x CUs + 11 one-segment trajectories: the launch is capped at 32 x CUs blocks of 8 groups (topt_grid), so the last 11 groups
    are taken in a second round of the grid-stride loop; every trajectory must carry the bytes of its copy in a call of one round."""
    torch, _ = dev()
    one_grid = 8 * 32 * torch.cuda.get_device_properties(0).multi_processor_count
    T, C = pool_of(golden, 4)
    nb = T.size
    lim = dict(depth=3, v_max=3.0, f_max=15.0, tilt_max=E.TILT_GOLDEN)
    small = device_call(gpu_ctx, 4, np.arange(nb + 1, dtype=np.int32), T, C.ravel(), uniform=1, **lim)
    n = one_grid + 11
    idx = np.arange(n) % nb
    big = device_call(gpu_ctx, 4, np.arange(n + 1, dtype=np.int32), T[idx], C[idx].ravel(), uniform=1, **lim)
    assert n * 8 > 64 * 32 * torch.cuda.get_device_properties(0).multi_processor_count
    for k in OUT:
        assert same_bytes(big[k], np.ascontiguousarray(small[k][idx])), k
    assert small["verdict"].any()


def test_status_non_finite_coefficients_and_null_outputs(gpu_ctx, golden):
    c = golden["r4-ragged"]
    st = np.array([1, 1, 3, 1], dtype=np.int32)
    got = run(gpu_ctx, c, depth=3, status=st, v_max=50.0)
    so = c["seg_offsets"]
    for b in (1, 2):
        sl = slice(int(so[b]), int(so[b + 1]))
        assert not got["range"][sl].any() and not got["norm"][sl].any() and not got["seg_verdict"][sl].any()
        assert not got["peak"][b].any() and got["verdict"][b] == 0
    assert E.decode(got["verdict"][0], "v_max") == "certified" and E.decode(got["verdict"][3], "v_max") == "certified"
    bad = c["coeff"].copy()
    bad[5] = np.nan          # trajectory 0, axis x, segment 0, t^5: velocity, acceleration and jerk of that axis
    bad[3 * 8 * 2 + 2] = np.inf   # trajectory 2 (offset 3 * 2r * 2), axis x, segment 0, t^2
    ref = reference(dict(c, coeff=bad), depth=2, v_max=1e6, a_max=1e6)
    nan = run(gpu_ctx, dict(c, coeff=bad), depth=2, v_max=1e6, a_max=1e6)
    assert np.array_equal(np.isfinite(nan["range"]), np.isfinite(ref["range"])) and np.array_equal(np.isfinite(nan["norm"]), np.isfinite(ref["norm"]))
    assert np.array_equal(np.isfinite(nan["peak"]), np.isfinite(ref["peak"]))
    assert not np.isfinite(nan["norm"][0, 0]).any() and not np.isfinite(nan["norm"][2, 1]).any()
    assert nan["seg_verdict"][0] == 0 and nan["verdict"][0] == 0 and nan["verdict"][2] == 0, "non-finite coefficients set no verdict bit"
    assert np.array_equal(nan["seg_verdict"], ref["seg_verdict"]) and np.array_equal(nan["verdict"], ref["verdict"])
    # a subset of the outputs: the same bytes as in the full call; no output at all: UAVQP_OK
    full = run(gpu_ctx, c, depth=3, v_max=2.0)
    for k in OUT:
        assert same_bytes(run(gpu_ctx, c, depth=3, v_max=2.0, want=(k,))[k], full[k]), k
    assert run(gpu_ctx, c, depth=3, want=()) == {}


def test_invalid_arguments(gpu_ctx, golden):
    c = golden["r4-M3"]
    L = _lib.lib()
    d_so, d_T, d_c = up(c["seg_offsets"]), up(c["times"]), up(c["coeff"])
    torch, d = dev()
    out = torch.zeros(3, dtype=torch.int32, device=d)
    box = torch.zeros((3, 3), dtype=torch.float64, device=d)

    def params(**kw):
        ep = _lib.EnvelopeParams()
        L.uavqp_default_envelope_params(ctypes.byref(ep))
        for k, v in kw.items():
            setattr(ep, k, v)
        return ep

    def call(r=4, n=1, uni=0, so=d_so, T=d_T, coeff=d_c, ep=None, lo=None, hi=None, ctx=gpu_ctx._h):
        ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
        return L.uavqp_envelope_device(ctx, r, n, uni, ptr(so), ptr(T), ptr(coeff), None, ctypes.byref(ep or params()), ptr(lo), ptr(hi),
                                       None, None, None, ptr(out), None)

    assert call() == _lib.UAVQP_OK and call(uni=3, so=None) == _lib.UAVQP_OK and call(lo=box, hi=box) == _lib.UAVQP_OK
    assert call(ep=params(f_min=3.0, f_max=3.0, tilt_max=1.5, depth=8)) == _lib.UAVQP_OK
    bad = [dict(r=2), dict(r=5), dict(n=-1), dict(uni=-1), dict(ep=params(struct_size=48)), dict(ep=params(depth=-1)), dict(ep=params(depth=9)),
           dict(T=None), dict(coeff=None), dict(so=None), dict(lo=box), dict(hi=box), dict(ep=params(f_min=5.0, f_max=4.0)),
           dict(ep=params(tilt_max=math.pi / 2)), dict(ep=params(tilt_max=2.0)), dict(ctx=None)]
    for name in ("v_max", "a_max", "j_max", "f_min", "f_max", "tilt_max"):
        bad += [dict(ep=params(**{name: -1.0})), dict(ep=params(**{name: math.inf})), dict(ep=params(**{name: math.nan}))]
    for kw in bad:
        assert call(**kw) == _lib.UAVQP_ERR_INVALID_ARG, kw
    gpu_ctx.synchronize()
    # the host entry refuses the same
    so, T, co = c["seg_offsets"], c["times"], c["coeff"]
    sv = np.zeros(3, dtype=np.int32)
    hb = np.zeros((3, 3))

    def hcall(r=4, n=1, uni=0, so=so, T=T, coeff=co, ep=None, lo=None, hi=None):
        ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        return L.uavqp_envelope_host(gpu_ctx._h, r, n, uni, ptr(so), ptr(T), ptr(coeff), None, ctypes.byref(ep or params()), ptr(lo), ptr(hi),
                                     None, None, None, ptr(sv), None)

    assert hcall() == _lib.UAVQP_OK
    for kw in (dict(r=5), dict(n=-1), dict(ep=params(depth=9)), dict(T=None), dict(so=None), dict(lo=hb), dict(ep=params(v_max=-1.0)),
               dict(ep=params(f_min=5.0, f_max=4.0))):
        assert hcall(**kw) == _lib.UAVQP_ERR_INVALID_ARG, kw
    none = L.uavqp_envelope_host(gpu_ctx._h, 4, 1, 0, so.ctypes.data, T.ctypes.data, co.ctypes.data, None, ctypes.byref(params()), None, None,
                                 None, None, None, None, None)
    assert none == _lib.UAVQP_OK


@pytest.mark.parametrize("name", ["r3-ragged", "r4-ragged", "r4-M9"])
def test_host_entry_equals_the_device_entry(gpu_ctx, golden, name):
    c = golden[name]
    n = len(c["times"])
    st = np.full(c["seg_offsets"].size - 1, U.UAVQP_SOLVED, dtype=np.int32)
    st[-1] = 2
    box = (np.full((n, 3), -3.0), np.full((n, 3), 4.0))
    lim = dict(depth=5, v_max=2.0, a_max=4.0, j_max=30.0, f_min=5.0, f_max=14.0, tilt_max=0.4)
    want = run(gpu_ctx, c, status=st, box=box, **lim)
    got = gpu_ctx.envelope(c["r"], c["seg_offsets"], c["times"], c["coeff"], status=st, box_lo=box[0], box_hi=box[1], **lim)
    for k, x in zip(OUT, got):
        assert same_bytes(x, want[k]), k


def test_end_to_end_sampled_peaks_lie_between_the_inner_and_the_outer_bound(gpu_ctx):
    """64 x 8 min-snap trajectories, one step of uavqp_time_reallocate_device at the default limits, solved again; uavqp_limit_penalty_device
    samples |v| and |a| at s T / 8 -- the leaf ends of depth 3.  Its peak is a value the quantity takes, so it cannot exceed outer_hi; and
    it is the largest over exactly the points inner_hi is taken over, so the two agree within the guard carried through the root.  What
    happens BETWEEN the samples is what the verdict adds: its counts are printed, not asserted."""
    import test_gpu_limit_penalty as LP
    lp = _lib.LimitParams()
    _lib.lib().uavqp_default_limit_params(ctypes.byref(lp))
    b = W.uniform_batch(2, 64, 8, 4, time_mode="distance")
    d = LP.Dev(gpu_ctx, b, True)
    d_T = d.up(d.T0)
    coeff, status = d.solve(d_T)
    gpu_ctx.time_reallocate_device(4, d.n, d.uni, None, d_T, coeff, lp.v_max, lp.a_max)
    coeff, status = d.solve(d_T)
    assert np.all(status.cpu().numpy() == U.UAVQP_SOLVED)
    peak = d.penalty(d_T, coeff, status=status, want=(False, False, False, True), samples_per_seg=8)[3].cpu().numpy()
    T, co = d_T.cpu().numpy(), coeff.cpu().numpy()
    got = device_call(gpu_ctx, 4, d.so, T, co, uniform=8, status=status.cpu().numpy(), depth=3, v_max=lp.v_max, a_max=lp.a_max)
    ref = E.envelope(4, d.so, T, co, depth=3)
    for k, lim in enumerate((lp.v_max, lp.a_max)):
        sampled = peak[:, k] * lim
        inner_hi, outer_hi = got["peak"][:, k, 2], got["peak"][:, k, 3]
        guard = (ref["Gq"][:, k] / (2 * ref["norm"][:, k, 2])).reshape(64, 8).max(axis=1)
        assert np.all(sampled <= outer_hi), k
        assert np.all(np.abs(sampled - inner_hi) <= guard + 4e-16 * sampled), (k, float(np.max(np.abs(sampled - inner_hi) / guard)))
    deep = device_call(gpu_ctx, 4, d.so, T, co, uniform=8, depth=6, v_max=lp.v_max, a_max=lp.a_max)
    for tag, res in (("depth 3", got), ("depth 6", deep)):
        for t in ("v_max", "a_max"):
            states = [E.decode(w, t) for w in res["verdict"]]
            print(f"end to end, {tag}, {t} = {getattr(lp, t)}: certified {states.count('certified')}, violated {states.count('violated')}, "
                  f"undecided {states.count('undecided')} of 64; sampled peak / limit <= {peak[:, 0 if t == 'v_max' else 1].max():.4f}, "
                  f"certified outer_hi / limit <= {res['peak'][:, 0 if t == 'v_max' else 1, 3].max() / getattr(lp, t):.4f}")


def facade_batch():
    b = W.uniform_batch(2, 6, 5, 4, time_mode="distance")
    return b, np.ascontiguousarray(b["seg_offsets"], dtype=np.int32)


def test_python_facade():
    b, so = facade_batch()
    opt = U.TrajOptimizer(order=4)
    opt.setWaypoints(b["waypoints"].reshape(-1, 3), wp_offsets=so + np.arange(so.size))
    opt.setTimeAllocation(b["times"].ravel())
    opt.setBoundary(b["bc"])
    with pytest.raises(U.UavqpError):
        opt.getEnvelope()
    assert opt.solve() is True
    env = opt.getEnvelope(depth=5, v_max=100.0, a_max=1e-3)
    ref = E.envelope(4, so, b["times"].ravel(), opt.getPolyCoeff(), depth=5, v_max=100.0, a_max=1e-3)
    ref["so"] = so
    assert_parity(env, ref, "facade")
    assert np.array_equal(env["verdict"], ref["verdict"]) and np.array_equal(env["seg_verdict"], ref["seg_verdict"])
    assert env["certified"]["v_max"].all() and env["violated"]["a_max"].all() and not env["undecided"]["v_max"].any()
    for t in ("j_max", "f_min", "f_max", "tilt_max", "box"):
        assert not env["certified"][t].any() and not env["violated"][t].any() and not env["undecided"][t].any(), "a test that is off"
    lo = np.full((30, 3), -1e3)
    boxed = opt.getEnvelope(box=(lo, -lo))
    assert boxed["certified"]["box"].all() and boxed["range"].shape == (30, 4, 3, 4)
    with pytest.raises(ValueError):
        opt.getEnvelope(rate_max=1.0)
    with pytest.raises(U.UavqpError):
        opt.getEnvelope(depth=9)


def test_cpp_facade_get_envelope(tmp_path):
    """TrajOptimizer::getEnvelope (cpp/traj_optimizer.h) agrees with uavqp_envelope_host byte for byte: tests/cpp/test_envelope_facade.cpp"""
    b, so = facade_batch()
    path = tmp_path / "batch.bin"
    with open(path, "wb") as fh:
        fh.write(np.array([4, so.size - 1, int(so[-1])], dtype=np.int32).tobytes())
        fh.write(so.tobytes())
        for key in ("waypoints", "times", "bc"):
            fh.write(np.ascontiguousarray(b[key], dtype=np.float64).tobytes())
    rocm = "/opt/rocm"
    exe = os.path.join(ROOT, "tests", "cpp", "test_envelope_facade")
    pkg = os.path.join(ROOT, "uav_motion_planning_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-I", os.path.join(rocm, "include"), f"-I{pkg}/cpp",
                           os.path.join(ROOT, "tests", "cpp", "test_envelope_facade.cpp"), f"-L{pkg}", "-luavqp", f"-Wl,-rpath,{pkg}",
                           f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib", "-o", exe])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "getEnvelope: 6 trajectories" in out.stdout
