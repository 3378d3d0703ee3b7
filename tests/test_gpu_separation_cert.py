"""-m gpu: the certified separation (uavqp_separation_certificate_device / _host) and its facades, against the numpy reference and the
mpmath truth of tests/separation_cert_reference.py.  The inputs -- batches, coefficients of the CPU oracle, clocks, d_req -- are those
tests/test_separation_cert_reference.py qualifies on the CPU.

Tolerances (derived, not measured).  Device and reference evaluate the same formulas in float64 and differ in contraction and in the order
of a sum only; the method bounds that rounding by the guards of the two entries and the allowance R of the pair arithmetic, so lower and
upper agree within the deciding pair's own allowance sqrt(3) max (G_i + G_j) + R (about 1e-12 m here).  Verdict words are EQUAL: d_req lies
more than two allowances from every bound (asserted on the reference).  `where` is EQUAL for every vehicle whose runner-up candidate is more
than two allowances from the winner.  Soundness against the truth has no tolerance.

Shapes.  95 vehicles in swarms of 2, 70, 1, 9, 4, 3 and 6 (tiles of 128, 3, 256, 28, 64, 85 and 42 leaves), uniform M = 8 and ragged M in
1..11, r = 3 / 4, depth 0 / 2 / 4 with 40 / 7 / 1 / 7 cells; one swarm of exactly 128 vehicles with M = 2 (a tile is 2 leaves)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import separation_cert_reference as C
import uav_motion_planning_amd as U
from uav_motion_planning_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = C.OUT
NONE = [-1, 0, -1, 0]


def dev():
    import torch
    return torch, torch.device("cuda", 0)


def up(x):
    torch, d = dev()
    return torch.from_numpy(np.ascontiguousarray(x)).to(d)


_COEFF = {}


def coeff_of(oracle, key, b):
    if key not in _COEFF:
        _COEFF[key] = C.solve(oracle, b)
    return _COEFF[key]


def device_call(ctx, r, so, T, coeff, go=None, start=None, uniform=0, status=None, want=OUT, guard=0, **params):
    """uavqp_separation_certificate_device on fresh device buffers pre-filled with NaN / -7 -> dict of numpy arrays; guard > 0: that many
    sentinel elements in front of and behind every output, returned with it"""
    torch, d = dev()
    so = np.ascontiguousarray(so, dtype=np.int32)
    n = so.size - 1
    ng = 1 if go is None else len(go) - 1
    shapes = dict(lower=n, upper=n, where=4 * n, verdict=n, group_verdict=ng)
    bufs = {k: (torch.full((shapes[k] + 2 * guard,), float("nan"), dtype=torch.float64, device=d) if k in ("lower", "upper")
                else torch.full((shapes[k] + 2 * guard,), -7, dtype=torch.int32, device=d)) if k in want else None for k in OUT}
    arg = {k: (None if v is None else v[guard:guard + shapes[k]]) for k, v in bufs.items()}
    d_so, d_T, d_c = up(so), up(np.asarray(T, dtype=np.float64)), up(np.asarray(coeff, dtype=np.float64))
    d_go = None if go is None else up(np.asarray(go, dtype=np.int32))
    d_start = None if start is None else up(np.asarray(start, dtype=np.float64))
    d_st = None if status is None else up(np.asarray(status, dtype=np.int32))
    torch.cuda.synchronize()
    ctx.separation_certificate_device(r, n, uniform, None if uniform else d_so, d_T, d_c, n_groups=ng, group_offsets=d_go, start=d_start,
                                      status=d_st, lower_out=arg["lower"], upper_out=arg["upper"], where_out=arg["where"],
                                      verdict_out=arg["verdict"], group_verdict_out=arg["group_verdict"], **params)
    ctx.synchronize()
    out = {k: v.cpu().numpy() for k, v in bufs.items() if v is not None}
    if "where" in out and not guard:
        out["where"] = out["where"].reshape(n, 4)
    return out


def call(ctx, b, co, **kw):
    return device_call(ctx, b["r"], b["so"], b["T"], co, go=b["go"], start=b["start"], **kw)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_parity(got, ref, tag):
    """words equal; lower / upper within the deciding pair's allowance; `where` equal where it is no tie.  -> the largest |difference| /
    allowance"""
    assert not np.any(got["verdict"] == -7) and not np.any(got["group_verdict"] == -7) and not np.any(got["where"] == -7), "every element is written"
    assert np.array_equal(got["verdict"], ref["verdict"]) and np.array_equal(got["group_verdict"], ref["group_verdict"]), tag
    worst = 0.0
    for k in ("lower", "upper"):
        g, w, allow = got[k], ref[k], ref["allow_" + k]
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w)), (tag, k)
        fin = np.isfinite(w)
        err = np.abs(g[fin] - w[fin])
        assert np.all(err <= allow[fin]), (tag, k, float(np.max(err - allow[fin])))
        with np.errstate(all="ignore"):
            ratio = np.where(allow[fin] > 0, err / allow[fin], 0.0)
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
    lo_ok, up_ok = C.where_comparable(ref)
    none = ref["where"][:, 0] < 0
    assert np.array_equal(got["where"][none], ref["where"][none]), tag
    assert np.array_equal(got["where"][lo_ok, :2], ref["where"][lo_ok, :2]), tag
    assert np.array_equal(got["where"][up_ok, 2:], ref["where"][up_ok, 2:]), tag
    return worst


@pytest.mark.parametrize("kind", sorted(C.GPU_KINDS))
def test_parity_with_the_reference(gpu_ctx, oracle, kind):
    b = C.gpu_batch(kind)
    co = coeff_of(oracle, kind, b)
    uni = 8 if C.GPU_KINDS[kind][1] else 0
    worst, classes = 0.0, set()
    for depth, n_cells in C.GPU_CLOCKS:
        clock = C.gpu_clock(depth, n_cells)
        ref = C.certificate(b["r"], b["so"], b["T"], co, group_offsets=b["go"], start=b["start"], **clock)
        assert C.two_allowances_away(ref, clock["d_req"])
        got = call(gpu_ctx, b, co, uniform=uni, **clock)
        worst = max(worst, assert_parity(got, ref, (kind, depth, n_cells)))
        classes |= {C.state(int(w)) for w in got["verdict"]}
    print(f"{kind}: worst |device - reference| = {worst:.3g} of the allowance")
    assert classes == {"certified", "violated", "undecided"}


@pytest.mark.parametrize("r", [3, 4])
def test_a_swarm_of_exactly_128_vehicles(gpu_ctx, oracle, r):
    b = C.full_swarm_batch(r)
    co = coeff_of(oracle, ("full", r), b)
    ref = C.certificate(r, b["so"], b["T"], co, group_offsets=b["go"], start=b["start"], **C.FULL_CLOCK)
    got = call(gpu_ctx, b, co, **C.FULL_CLOCK)
    worst = assert_parity(got, ref, ("full", r))
    print(f"128 vehicles r={r}: worst |device - reference| = {worst:.3g} of the allowance")
    alone = device_call(gpu_ctx, r, b["so"], b["T"], co, go=None, start=b["start"], uniform=2, **C.FULL_CLOCK)   # NULL offsets: one swarm
    for k in OUT:
        assert same_bytes(alone[k], got[k]), k


@pytest.mark.parametrize("r,downwash", [(3, 1.0), (4, 1.5)])
def test_device_output_is_sound_against_the_truth(gpu_ctx, oracle, r, downwash):
    """lower <= truth at 64 instants of every depth-3 leaf and truth(witness) <= upper on the DEVICE's own numbers, no tolerance"""
    b, clock = C.small_batch(r, downwash)
    co = coeff_of(oracle, ("small", r), b)
    tr = C.truth(r, b["so"], b["T"], co, group_offsets=b["go"], start=b["start"], **clock)
    bad = []
    for depth in (0, 2, 5):
        got = call(gpu_ctx, b, co, **dict(clock, depth=depth))
        bad += C.soundness_failures(got, tr, C.taus(depth, clock["n_cells"], clock["clock_start"], clock["dt"]), f"device r={r} depth={depth}")
        for i, m in enumerate(tr[0]):
            if m is not None:
                assert not (got["verdict"][i] & C.CERTIFIED) or m >= clock["d_req"]
    assert not bad, "\n".join(bad[:20])


def sub_batch(b, co, g):
    """swarm g of a batch as a batch of its own"""
    r, so, go = b["r"], b["so"], b["go"]
    t0, t1 = int(go[g]), int(go[g + 1])
    s0, s1 = int(so[t0]), int(so[t1])
    return (dict(r=r, so=(so[t0:t1 + 1] - s0).astype(np.int32), T=b["T"][s0:s1], go=np.array([0, t1 - t0], dtype=np.int32), start=b["start"][t0:t1]),
            co[3 * 2 * r * s0:3 * 2 * r * s1], slice(t0, t1))


@pytest.mark.parametrize("kind", ["ragged_M1to11_r3", "uniform_M8_r4"])
def test_byte_identity(gpu_ctx, oracle, kind, monkeypatch):
    """a second run; a swarm alone against the same swarm in the middle of the batch; the grid stride (two blocks for seven swarms); NULL
    subsets of the outputs; the host entry"""
    b = C.gpu_batch(kind)
    co = coeff_of(oracle, kind, b)
    clock = C.gpu_clock(2, 7)
    st = np.full(b["so"].size - 1, U.UAVQP_SOLVED, dtype=np.int32)
    st[[5, 80]] = 2
    full = call(gpu_ctx, b, co, status=st, **clock)
    again = call(gpu_ctx, b, co, status=st, **clock)
    for k in OUT:
        assert same_bytes(full[k], again[k]), k
    for g in (1, 3):
        sb, sc, sl = sub_batch(b, co, g)
        alone = call(gpu_ctx, sb, sc, status=st[sl], **clock)
        assert same_bytes(alone["lower"], full["lower"][sl]) and same_bytes(alone["upper"], full["upper"][sl])
        assert same_bytes(alone["verdict"], full["verdict"][sl]) and alone["group_verdict"][0] == full["group_verdict"][g]
        shift = np.where(alone["where"][:, [0, 2]] >= 0, sl.start, 0)
        assert np.array_equal(alone["where"][:, [0, 2]] + shift, full["where"][sl][:, [0, 2]])
        assert np.array_equal(alone["where"][:, [1, 3]], full["where"][sl][:, [1, 3]])
    for k in OUT:
        assert same_bytes(call(gpu_ctx, b, co, status=st, want=(k,), **clock)[k], full[k]), k
    assert call(gpu_ctx, b, co, status=st, want=(), **clock) == {}
    host = gpu_ctx.separation_certificate(b["r"], b["so"], b["T"], co, group_offsets=b["go"], start=b["start"], status=st, **clock)
    for k, x in zip(OUT, host):
        assert same_bytes(x, full[k]), k
    monkeypatch.setenv("UAVQP_SEPARATION_CERT_BLOCKS", "2")
    ctx2 = U.Context(0)
    try:
        small = call(ctx2, b, co, status=st, **clock)
    finally:
        ctx2.close()
    for k in OUT:
        assert same_bytes(small[k], full[k]), k


def test_an_oversize_swarm(gpu_ctx):
    """129 vehicles: the host entry refuses the swarm; the device entry gives it NaN bounds and zero words, and evaluates its neighbours"""
    r, n = 3, 129 + 2
    rng = np.random.default_rng(9)
    so = np.arange(n + 1, dtype=np.int32)
    T = np.full(n, 1.0)
    co = rng.uniform(-1.0, 1.0, size=3 * 2 * r * n)
    go = np.array([0, 129, 131], dtype=np.int32)
    clock = dict(depth=1, n_cells=3, clock_start=0.0, dt=0.4, d_req=0.5)
    got = device_call(gpu_ctx, r, so, T, co, go=go, **clock)
    assert np.isnan(got["lower"][:129]).all() and np.isnan(got["upper"][:129]).all() and not got["verdict"][:129].any()
    assert got["group_verdict"][0] == 0 and np.all(got["where"][:129] == NONE)
    ref = C.certificate(r, so, T, co, group_offsets=go, **clock)
    assert np.isfinite(got["lower"][129:]).all() and np.array_equal(got["verdict"][129:], ref["verdict"][129:])
    with pytest.raises(U.UavqpError):
        gpu_ctx.separation_certificate(r, so, T, co, group_offsets=go, **clock)
    with pytest.raises(U.UavqpError):
        gpu_ctx.separation_certificate(r, so, T, co, **clock)      # NULL offsets: one swarm of 131


def test_status_mask_non_finite_coefficients_and_guard_elements(gpu_ctx, oracle):
    b, clock = C.small_batch(4, 1.5)
    co = coeff_of(oracle, ("small", 4), b)
    so, go = b["so"], b["go"]
    n = so.size - 1
    st = np.full(n, U.UAVQP_SOLVED, dtype=np.int32)
    st[[1, 3]] = [3, 0]      # the second vehicle of the pair; one of the three
    ref = C.certificate(4, so, b["T"], co, group_offsets=go, start=b["start"], status=st, **clock)
    got = call(gpu_ctx, b, co, status=st, guard=3, **clock)
    for k in OUT:      # three sentinels in front and behind
        fill = got[k][:3]
        assert (np.isnan(fill).all() if k in ("lower", "upper") else np.all(fill == -7)) and same_bytes(got[k][:3], got[k][-3:]), k
        got[k] = got[k][3:-3]
    got["where"] = got["where"].reshape(n, 4)
    assert_parity(got, ref, "status")
    for t in (1, 3):
        assert got["lower"][t] == np.inf and got["upper"][t] == np.inf and got["where"][t].tolist() == NONE and got["verdict"][t] == 0
    assert got["lower"][0] == np.inf and got["verdict"][0] & C.CERTIFIED and got["where"][0].tolist() == NONE, "its only partner did not solve"
    assert got["group_verdict"][0] & C.CERTIFIED
    assert np.isfinite(got["lower"][2]) and got["where"][2, 0] == 4 and got["where"][2, 2] == 4, "the swarm of three goes on as a pair"
    # non-finite coefficients: the vehicle and its partners
    bad = co.copy()
    s5 = int(so[5])
    bad[3 * 8 * s5 + 3] = np.nan           # vehicle 5 (the swarm of five), axis x, segment 0
    bad[3 * 8 * int(so[2]) + 8 * int(so[3] - so[2]) + 1] = np.inf      # vehicle 2 (the swarm of three), axis y, segment 0
    got = call(gpu_ctx, b, bad, **clock)
    ref = C.certificate(4, so, b["T"], bad, group_offsets=go, start=b["start"], **clock)
    assert_parity(got, ref, "non-finite")
    for t in range(2, 10):
        assert np.isnan(got["lower"][t]) and np.isnan(got["upper"][t]) and got["verdict"][t] == 0 and got["where"][t].tolist() == NONE, t
    assert got["group_verdict"][1] == 0 and got["group_verdict"][2] == 0
    assert np.isfinite(got["lower"][:2]).all() and got["lower"][10] == np.inf


def test_invalid_arguments(gpu_ctx, oracle):
    b, _ = C.small_batch(4, 1.5)
    co = coeff_of(oracle, ("small", 4), b)
    L = _lib.lib()
    so, go, T, start = b["so"], b["go"], b["T"], b["start"]
    n, ng = so.size - 1, go.size - 1
    d_so, d_go, d_T, d_c, d_s = up(so), up(go), up(T), up(co), up(start)
    torch, d = dev()
    out = torch.zeros(n, dtype=torch.int32, device=d)

    def params(**kw):
        sp = _lib.SeparationParams()
        L.uavqp_default_separation_params(ctypes.byref(sp))
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp

    def dcall(r=4, n=n, uni=0, so=d_so, T=d_T, coeff=d_c, ng=ng, go=d_go, sp=None, ctx=gpu_ctx._h):
        ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
        return L.uavqp_separation_certificate_device(ctx, r, n, uni, ptr(so), ptr(T), ptr(coeff), None, ng, ptr(go), d_s.data_ptr(),
                                                     ctypes.byref(sp or params()), None, None, None, ptr(out), None)

    sv = np.zeros(n, dtype=np.int32)

    def hcall(r=4, n=n, uni=0, so=so, T=T, coeff=co, ng=ng, go=go, sp=None, ctx=gpu_ctx._h):
        ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        return L.uavqp_separation_certificate_host(ctx, r, n, uni, ptr(so), ptr(T), ptr(coeff), None, ng, ptr(go), start.ctypes.data,
                                                   ctypes.byref(sp or params()), None, None, None, ptr(sv), None)

    bad = [dict(r=2), dict(r=5), dict(n=-1), dict(uni=-1), dict(ng=-1), dict(go=None), dict(sp=params(struct_size=40)), dict(sp=params(struct_size=0)),
           dict(sp=params(depth=-1)), dict(sp=params(depth=7)), dict(sp=params(n_cells=0)), dict(sp=params(n_cells=-3)),
           dict(sp=params(n_cells=(1 << 20) + 1)), dict(sp=params(d_req=0.0)), dict(sp=params(d_req=-0.5)), dict(sp=params(d_req=math.inf)),
           dict(sp=params(d_req=math.nan)), dict(sp=params(dt=0.0)), dict(sp=params(dt=math.inf)), dict(sp=params(downwash=0.5)),
           dict(sp=params(downwash=math.nan)), dict(sp=params(clock_start=math.inf)), dict(T=None), dict(coeff=None), dict(so=None), dict(ctx=None)]
    for entry in (dcall, hcall):
        assert entry() == _lib.UAVQP_OK
        assert entry(sp=params(depth=0, d_req=1e-9)) == _lib.UAVQP_OK and entry(sp=params(depth=6, n_cells=2, d_req=1e9)) == _lib.UAVQP_OK
        for kw in bad:
            assert entry(**kw) == _lib.UAVQP_ERR_INVALID_ARG, (entry.__name__, kw)
        gpu_ctx.synchronize()
    # the offsets the host entry validates
    for wrong in ([1, 2, 5, 10, 11], [0, 2, 5, 10, 12], [0, 5, 2, 10, 11]):
        assert hcall(go=np.array(wrong, dtype=np.int32)) == _lib.UAVQP_ERR_INVALID_ARG, wrong
    # no output at all: nothing to do, whatever the pointers
    none = L.uavqp_separation_certificate_host(gpu_ctx._h, 4, n, 0, so.ctypes.data, T.ctypes.data, co.ctypes.data, None, ng, go.ctypes.data, None,
                                               ctypes.byref(params()), None, None, None, None, None)
    assert none == _lib.UAVQP_OK


def test_python_facade(oracle):
    b, clock = C.small_batch(4, 1.5)
    so = np.ascontiguousarray(b["so"], dtype=np.int32)
    opt = U.TrajOptimizer(order=4)
    opt.setWaypoints(b["wp"], wp_offsets=so + np.arange(so.size))
    opt.setTimeAllocation(b["T"])
    opt.setBoundary(b["bc"])
    opt.setSwarm(b["go"], b["start"])
    with pytest.raises(U.UavqpError):
        opt.getSeparationCertificate()      # nothing solved yet
    assert opt.solve() is True
    kw = {k: v for k, v in clock.items() if k != "d_req"}
    cert = opt.getSeparationCertificate(depth=3, d_req=clock["d_req"], **kw)
    ref = C.certificate(4, so, b["T"], opt.getPolyCoeff(), group_offsets=b["go"], start=b["start"], **dict(clock, depth=3))
    assert C.two_allowances_away(ref, clock["d_req"])
    assert_parity(cert, ref, "facade")
    assert cert["lower"].shape == (11,) and cert["where"].shape == (11, 4) and cert["group_verdict"].shape == (4,)
    assert np.array_equal(cert["certified"], (cert["verdict"] & 1) != 0) and np.array_equal(cert["violated"], (cert["verdict"] & 2) != 0)
    assert np.array_equal(cert["undecided"], ~cert["certified"] & ~cert["violated"]) and np.array_equal(cert["moving"], (cert["verdict"] & 4) != 0)
    assert not np.any(cert["certified"] & cert["violated"]) and cert["certified"][10], "the swarm of one is certified"
    assert opt.getSeparationCertificate(depth=0, d_req=100.0, **kw)["violated"][:10].all()
    with pytest.raises(U.UavqpError):
        opt.getSeparationCertificate(depth=7)
    with pytest.raises(U.UavqpError):
        opt.getSeparationCertificate(d_req=0.0)
    with pytest.raises(ValueError):
        opt.getSeparationCertificate(d_safe=1.0)      # no field of uavqp_separation_params


def test_cpp_facade_get_separation_certificate():
    """TrajOptimizer::getSeparationCertificate (cpp/traj_optimizer.h) agrees with uavqp_separation_certificate_host byte for byte:
    tests/cpp/test_separation_cert_facade.cpp"""
    rocm = "/opt/rocm"
    exe = os.path.join(ROOT, "tests", "cpp", "test_separation_cert_facade")
    pkg = os.path.join(ROOT, "uav_motion_planning_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-I", os.path.join(rocm, "include"), f"-I{pkg}/cpp",
                           os.path.join(ROOT, "tests", "cpp", "test_separation_cert_facade.cpp"), f"-L{pkg}", "-luavqp", f"-Wl,-rpath,{pkg}",
                           f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "getSeparationCertificate: words 2" in out.stdout


def test_end_to_end_after_the_swarm_optimiser(gpu_ctx):
    """16 swarms of 4 crossing vehicles with 8 segments through uavqp_swarm_optimize_host, then the certificate of the result.  depth 0 on
    the penalty's clock: upper, less the allowance it carries, is the optimiser's sampled min_sep within the allowance (swarms with no sample within 1e-3 s of a knot:
    the penalty's segment rule keeps a sample on the earlier segment for 1e-4 s past a knot).  depth 4: lower <= truth <= upper on four of
    the swarms.  The unoptimised crossing: the violated bit for every vehicle whose sampled separation is already below d_req."""
    import spacetime_reference as R
    import swarm_opt_reference as O
    import waypoint_opt_reference as W
    from uav_motion_planning_amd.esdf import EsdfMap
    r = 4
    b = O.batch(r, ((8,) * 4,) * 16, 4242)
    so, go = b["seg_offsets"], b["group_offsets"]
    sw = O.SWARM
    clock = dict(n_cells=sw["n_samples"], clock_start=sw["clock_start"], dt=sw["dt"], downwash=sw["downwash"], d_req=sw["d_safe"])
    with EsdfMap(gpu_ctx, W.DIMS, W.ORIGIN, W.RES, W.MAX_DIST) as m:
        m.set_occupancy(R.scene()["occ"])
        m.update()
        kw = dict(group_offsets=go, start=b["start"], limits=O.LIMITS, clearance=R.CLEARANCE, swarm=sw, max_move=O.PARAMS["max_move"])
        res0 = gpu_ctx.swarm_optimize_host(r, so, b["waypoints"].copy(), b["times"].copy(), b["bc"], m, max_iters=0, **kw)
        res = gpu_ctx.swarm_optimize_host(r, so, b["waypoints"].copy(), b["times"].copy(), b["bc"], m, **kw)
    for (wp, T, start, coeff, status, _, _, _, _, _, min_sep), optimised in ((res0, False), (res, True)):
        assert np.all(status == U.UAVQP_SOLVED)
        lower, upper, where, verdict, gv = gpu_ctx.separation_certificate(r, so, T, coeff, group_offsets=go, start=start, status=status, depth=0, **clock)
        if not optimised:
            crossing = min_sep < clock["d_req"] - 1e-9
            assert crossing.sum() >= 32 and np.all(verdict[crossing] & C.VIOLATED), "the straight-line crossing is violated at its samples already"
            continue
        ref = C.certificate(r, so, T, coeff, group_offsets=go, start=start, depth=0, **clock)
        tw = C.taus(0, clock["n_cells"], clock["clock_start"], clock["dt"])
        clear = np.array([np.min(np.abs(np.array(C.knots(T[so[t]:so[t + 1]], start[t]))[:, None] - tw[None, :])) > 1e-3 for t in range(64)])
        ok = np.repeat(clear.reshape(16, 4).all(axis=1), 4)
        assert ok.sum() >= 8, "some swarms have no sample within 1e-3 s of a knot (36 knots per swarm: about half of them do)"
        # upper = s + allowance by definition (s the separation at the witness), so it is s = upper - allowance that is the penalty's sampled
        # min_sep within the allowance; upper itself lies ABOVE min_sep by the allowance to the last bits (measured 5.694e-13 against
        # 5.693e-13), never below it
        s_wit = upper[ok] - ref["allow_upper"][ok]
        print(f"end to end: |upper - allowance - min_sep| at most {np.max(np.abs(s_wit - min_sep[ok])):.3g}, allowance {ref['allow_upper'][ok].min():.3g}")
        assert np.all(np.abs(s_wit - min_sep[ok]) <= ref["allow_upper"][ok]) and np.all(upper[ok] >= min_sep[ok])
        assert np.all(lower <= upper)
        # depth 4 against the truth, on the first four swarms
        sel = slice(0, 16)
        s1 = int(so[16])
        sub = dict(r=r, so=so[:17], T=T[:s1], go=go[:5], start=start[:16])
        got = call(gpu_ctx, sub, coeff[:3 * 2 * r * s1], **dict(clock, depth=4))
        l4, u4, _, _, _ = gpu_ctx.separation_certificate(r, so, T, coeff, group_offsets=go, start=start, status=status, depth=4, **clock)
        assert same_bytes(got["lower"], l4[sel]) and same_bytes(got["upper"], u4[sel])
        tr = C.truth(r, sub["so"], sub["T"], coeff[:3 * 2 * r * s1], group_offsets=sub["go"], start=sub["start"], per_leaf=2, **clock)
        assert C.soundness_failures(got, tr, C.taus(4, clock["n_cells"], clock["clock_start"], clock["dt"]), "end to end") == []
        states = [C.state(int(w)) for w in verdict]
        print(f"end to end at d_req {clock['d_req']}: depth 0 certified {states.count('certified')}, violated {states.count('violated')}, undecided "
              f"{states.count('undecided')} of 64; sampled min_sep {min_sep.min():.3f} .. {min_sep.max():.3f}, lower at depth 4 {l4.min():.3f} .. {l4.max():.3f}")
