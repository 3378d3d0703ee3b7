"""-m gpu: the joint optimiser with the attitude penalty in its objective (uavqp_attitude_optimize_device / _host) and its facades, against
uavqp_spacetime_lbfgs_device, the separate entries, and the recorded optima of scipy's L-BFGS-B on the CPU reference objective
(tests/attitude_opt_reference.py, tests/golden/attitude_scipy.json).

Scene, harness and batches are those of tests/test_gpu_spacetime_lbfgs.py (imported, not copied) at AO.TIME_SCALE x their durations: the
ragged batch of 14 trajectories plus the designed invalid one at r = 3, the uniform batch of 8 x 4 segments at r = 4; max_move = 1 m.

Bounds.  All attitude weights zero: every output byte-equal to uavqp_spacetime_lbfgs_device.  objective[:, 1] against f recomputed from the
returned waypoints and durations through the separate entries (solve, cost, flight penalty, attitude penalty): 1e-9 relative.  Against
scipy: gap = (f_lib - f_scipy) / (f_start - f_scipy) <= 4 x AO.GAP_ATTITUDE_AT_DEFAULT at the default 32 trials, on cases with
f_start > 1.5 f_scipy, no trajectory left out except the designed invalid one; the factor 4 and its reason are those of
tests/test_gpu_spacetime_lbfgs.py (CPU perturbations far larger than rounding moved the transcription's worst gap by up to 2.3 x; doubling
that leaves room for another floating-point order).  Everything else is exact."""
import json
import os
import subprocess

import numpy as np
import pytest

import uav_motion_planning_amd as U
from uav_motion_planning_amd.esdf import EsdfMap

import attitude_opt_reference as AO
import spacetime_reference as R
import test_gpu_spacetime as G
import test_gpu_spacetime_lbfgs as B
import waypoint_opt_reference as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attitude_scipy.json")
MOVE = G.MOVE
GAP_BOUND = 4.0 * AO.GAP_ATTITUDE_AT_DEFAULT
OUT_KEYS = G.OUT_KEYS + ("apk",)
OFF = dict(weight_thrust=0.0, weight_tilt=0.0, weight_rate=0.0)
IDS = [f"r{r}-{k}" for r, k in AO.KINDS]


@pytest.fixture(scope="module")
def esdf(gpu_ctx):
    sc = R.scene()
    m = EsdfMap(gpu_ctx, W.DIMS, W.ORIGIN, W.RES, W.MAX_DIST)
    m.set_occupancy(sc["occ"])
    m.update()
    gpu_ctx.synchronize()
    yield m
    m.close()


class Dev(B.Dev):
    """The harness of tests/test_gpu_spacetime_lbfgs.py with the new entry beside uavqp_spacetime_lbfgs_device (lbfgs)."""

    def attitude_opt(self, esdf, attitude=None, null=(), **params):
        t = self.torch
        d_wp, d_T = self.up(self.wp0), self.up(self.T0)
        out = dict(coeff=self.zeros(3 * 2 * self.r * self.total), status=self.zeros(self.n, t.int32), obj=self.zeros((self.n, 2)),
                   acc=self.zeros(self.n, t.int32), peak=self.zeros((self.n, 2)), md=self.zeros(self.n), outside=self.zeros(self.n, t.int32),
                   apk=self.zeros((self.n, 4)) + float("nan"))
        params.setdefault("max_move", MOVE)
        arg = {k: (None if k in null else v) for k, v in out.items()}
        t.cuda.synchronize()
        self.ctx.attitude_optimize_device(self.r, self.n, self.uni, self.mmax, self.total, self.d_so, d_wp, d_T, self.d_bc, esdf, arg["coeff"],
                                          arg["status"], arg["obj"], arg["acc"], arg["peak"], arg["md"], arg["outside"], arg["apk"],
                                          limits=dict(R.LIMITS_OF[self.r]), clearance=dict(R.CLEARANCE),
                                          attitude=dict(AO.ATTITUDE, **(attitude or {})), **params)
        self.ctx.synchronize()
        res = {k: v.cpu().numpy() for k, v in out.items()}
        res["wp"], res["T"] = d_wp.cpu().numpy(), d_T.cpu().numpy()
        res["d_wp"], res["d_T"] = d_wp, d_T
        return res

    def attitude_penalty(self, d_T, coeff, status, **params):
        t = self.torch
        phi, pk = self.zeros(self.n) + float("nan"), self.zeros((self.n, 4)) + float("nan")
        t.cuda.synchronize()
        self.ctx.attitude_penalty_device(self.r, self.n, self.uni, self.d_so, d_T, coeff, status=status, penalty=phi, peak=pk,
                                         **dict(AO.ATTITUDE, **params))
        self.ctx.synchronize()
        return phi.cpu().numpy(), pk.cpu().numpy()

    def cost(self, d_T, coeff):
        cost, grad = self.zeros(self.n), self.zeros(self.total)
        self.torch.cuda.synchronize()
        self.ctx.cost_time_gradient_device(self.r, self.n, self.uni, self.d_so, d_T, coeff, cost, grad)
        self.ctx.synchronize()
        return cost.cpu().numpy()


_runs = {}


def run_of(gpu_ctx, esdf, r, kind):
    """The default-parameter run of one of the two batches (computed once per module): (Dev, result, index of the invalid trajectory)."""
    if (r, kind) not in _runs:
        if kind == "ragged":
            b, bad = G.with_invalid(AO.batch_of(r, kind))
            d = Dev(gpu_ctx, b, False)
        else:
            d, bad = Dev(gpu_ctx, AO.batch_of(r, kind), True), None
        _runs[(r, kind)] = (d, d.attitude_opt(esdf), bad)
    return _runs[(r, kind)]


@pytest.mark.parametrize("r,kind", AO.KINDS, ids=IDS)
def test_with_all_attitude_weights_zero_every_byte_is_the_lbfgs_entrys(gpu_ctx, esdf, r, kind):
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    plain = d.lbfgs(esdf)
    off = d.attitude_opt(esdf, attitude=OFF)
    for k in G.OUT_KEYS:
        assert plain[k].tobytes() == off[k].tobytes(), k
    # ... while the peaks are still reported, and with the weights on the result is another one
    fresh, st = d.solve(off["d_wp"], off["d_T"])
    assert off["apk"].tobytes() == d.attitude_penalty(off["d_T"], fresh, st, **OFF)[1].tobytes()
    ok = G.valid_ids(d, bad)
    assert np.all(res["obj"][ok, 0] > plain["obj"][ok, 0])
    for t in ok:
        assert np.any(res["T"][d.so[t]:d.so[t + 1]] != plain["T"][d.so[t]:d.so[t + 1]]), f"trajectory {t} ignores the attitude penalty"


@pytest.mark.parametrize("r,kind", AO.KINDS, ids=IDS)
def test_attitude_optimiser_contract(gpu_ctx, esdf, r, kind):
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    P = B.defaults()
    ok = G.valid_ids(d, bad)
    st = res["status"]
    assert np.all(st[ok] == U.UAVQP_SOLVED)
    assert np.all(res["obj"][ok, 1] <= res["obj"][ok, 0]), "f never increases"
    assert np.all(res["acc"][ok] > 0) and np.all(res["acc"] <= P.max_iters) and np.all(res["obj"][ok, 1] < res["obj"][ok, 0])
    assert np.all(res["wp"] >= d.wp0 - MOVE) and np.all(res["wp"] <= d.wp0 + MOVE)
    if bad is not None:     # the designed invalid trajectory comes back untouched
        k0, k1, s0, s1 = int(d.so[bad]) + bad, int(d.so[bad + 1]) + bad, int(d.so[bad]), int(d.so[bad + 1])
        assert st[bad] == U.UAVQP_INVALID_INPUT and res["acc"][bad] == 0 and np.all(np.isnan(res["obj"][bad]))
        assert res["wp"][k0:k1 + 1].tobytes() == d.wp0[k0:k1 + 1].tobytes() and res["T"][s0:s1].tobytes() == d.T0[s0:s1].tobytes()
        assert tuple(res["apk"][bad]) == (0.0, np.inf, 0.0, 0.0)
    # the coefficients and the status are a plain solve at the point handed back, bit for bit
    fresh, st2 = d.solve(res["d_wp"], res["d_T"])
    assert fresh.cpu().numpy().tobytes() == res["coeff"].tobytes() and np.array_equal(st2.cpu().numpy(), st)
    # the objective recomputed through the separate entries
    J = d.cost(res["d_T"], fresh)
    pen = d.flight(esdf, res["d_T"], fresh, st2, want=("phi", "peak", "min_dist", "outside"))
    phi_att, apk = d.attitude_penalty(res["d_T"], fresh, st2)
    f = P.smooth_weight * J + P.time_weight * np.add.reduceat(res["T"], d.so[:-1]) + pen["phi"] + phi_att
    err = float(np.max(np.abs(f[ok] - res["obj"][ok, 1]) / res["obj"][ok, 1]))
    print(f"r={r} {kind}: objective at the result against the separate entries: {err:.3e}; median f_result / f_start "
          f"{np.median(res['obj'][ok, 1] / res['obj'][ok, 0]):.3e}; attitude peaks at the result, max: {res['apk'][ok].max(axis=0)}")
    assert err <= 1e-9
    assert apk.tobytes() == res["apk"].tobytes() and pen["peak"].tobytes() == res["peak"].tobytes() and pen["min_dist"].tobytes() == res["md"].tobytes()
    # the start objective is that of the plain entry plus the attitude penalty of the start
    c0, st0 = d.solve(d.up(d.wp0), d.up(d.T0))
    phi0, apk0 = d.attitude_penalty(d.up(d.T0), c0, st0)
    plain0 = d.lbfgs(esdf, max_iters=0)
    assert np.max(np.abs(plain0["obj"][ok, 0] + phi0[ok] - res["obj"][ok, 0]) / res["obj"][ok, 0]) <= 1e-12
    # tilt and body rate start outside the limits on every trajectory and end closer to them
    assert np.all(apk0[ok, 3] > AO.ATTITUDE["rate_max"]) and np.all(res["apk"][ok, 3] < apk0[ok, 3])
    over = apk0[ok, 2] > AO.ATTITUDE["tilt_max"]
    assert np.count_nonzero(over) * 2 >= len(ok) and np.all(res["apk"][ok, 2][over] < apk0[ok, 2][over])
    # run to run: identical bytes; the host entry; NULL outputs
    again = d.attitude_opt(esdf)
    for k in OUT_KEYS:
        assert res[k].tobytes() == again[k].tobytes(), k
    host = gpu_ctx.attitude_optimize_host(r, d.so, d.wp0, d.T0, d.bc0, esdf, uniform_segments=d.uni, limits=R.LIMITS_OF[r], clearance=R.CLEARANCE,
                                          attitude=AO.ATTITUDE, max_move=MOVE)
    for k, v in zip(OUT_KEYS, host):
        assert res[k].tobytes() == v.tobytes(), k
    part = d.attitude_opt(esdf, null=("status", "acc", "peak", "md", "outside", "apk"))
    for k in ("wp", "T", "coeff", "obj"):
        assert part[k].tobytes() == res[k].tobytes(), k
    # max_iters = 0: the plain solve, both objective columns equal and holding the penalty
    z = d.attitude_opt(esdf, max_iters=0)
    assert z["wp"].tobytes() == d.wp0.tobytes() and z["coeff"].tobytes() == c0.cpu().numpy().tobytes() and np.all(z["acc"] == 0)
    assert np.array_equal(z["obj"][ok, 0], z["obj"][ok, 1]) and np.array_equal(z["obj"][ok, 0], res["obj"][ok, 0]) and z["apk"].tobytes() == apk0.tobytes()


@pytest.mark.parametrize("r,kind", AO.KINDS, ids=IDS)
def test_attitude_optimiser_vs_scipy_lbfgsb(gpu_ctx, esdf, r, kind):
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    assert B.defaults().max_iters == AO.DEFAULT_MAX_ITERS
    golden = json.load(open(GOLDEN))[f"r{r}-{kind}"]
    gaps = []
    for t in G.valid_ids(d, bad):
        rec = golden[G.original_index(t, bad)]
        f_start, f_scipy = res["obj"][t, 0], rec["f_scipy"]
        assert abs(f_start - rec["f_start"]) <= 1e-9 * f_start, "the recorded results belong to other cases"
        assert rec["outside"] == 0 and res["outside"][t] == 0
        assert f_start > 1.5 * f_scipy, "the case has no decrease to speak of"
        gaps.append((res["obj"][t, 1] - f_scipy) / (f_start - f_scipy))
    print(f"r={r} {kind}: {len(gaps)} trajectories at max_iters = {AO.DEFAULT_MAX_ITERS}: worst gap {max(gaps):.3e} (trajectory "
          f"{int(np.argmax(gaps))}; bound {GAP_BOUND:.3e}); all: " + " ".join(f"{g:.1e}" for g in gaps))
    assert len(gaps) == d.n - (0 if bad is None else 1) == len(golden), "no trajectory is left out except the designed invalid one"
    for t, gap in zip(G.valid_ids(d, bad), gaps):
        assert gap <= GAP_BOUND, f"r={r} {kind} trajectory {t}: gap {gap:.3e}"


def test_attitude_optimiser_refuses_invalid_attitude_params(gpu_ctx, esdf):
    d, _, _ = run_of(gpu_ctx, esdf, 4, "uniform")
    for bad in (dict(samples_per_seg=0), dict(gravity=0.0), dict(f_min=-1.0), dict(f_min=11.0, f_max=10.0), dict(f_max=np.inf),
                dict(tilt_max=0.0), dict(tilt_max=1.6), dict(rate_max=0.0), dict(weight_thrust=-1.0), dict(weight_tilt=np.nan),
                dict(weight_rate=np.inf)):
        with pytest.raises(U.UavqpError):
            d.attitude_opt(esdf, attitude=bad)
    with pytest.raises(ValueError):
        d.attitude_opt(esdf, attitude=dict(no_such_field=1.0))
    with pytest.raises(U.UavqpError):
        d.attitude_opt(esdf, memory=0)
    with pytest.raises(U.UavqpError):
        d.attitude_opt(esdf, null=("obj",))


def test_python_facade_optimize_trajectory_attitude():
    b = AO.batch_of(3, "ragged")
    so = b["seg_offsets"]
    lim, clr, par = dict(R.LIMITS_OF[3]), dict(R.CLEARANCE), dict(max_move=MOVE, memory=4)
    opt = U.TrajOptimizer(order=3)
    opt.setWaypoints(b["waypoints"], wp_offsets=so + np.arange(so.size))
    opt.setTimeAllocation(b["times"])
    opt.setBoundary(b["bc"])
    ctx = opt.context()
    sc = R.scene()
    with EsdfMap(ctx, W.DIMS, W.ORIGIN, W.RES, W.MAX_DIST) as m:
        m.set_occupancy(sc["occ"])
        m.update()
        want = ctx.attitude_optimize_host(3, so, b["waypoints"], b["times"], b["bc"], m, limits=lim, clearance=clr, attitude=AO.ATTITUDE, **par)
        assert opt.optimizeTrajectoryAttitude(m, limits=lim, clearance=clr, attitude=AO.ATTITUDE, **par) is True
        got = (opt.getWaypoints(), opt.getTimeAllocation(), opt.getPolyCoeff(), opt.status, opt.objective, opt.iterations, opt.peak, opt.min_dist,
               opt.outside, opt.attitude_peak)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        assert np.all(opt.objective[:, 1] < opt.objective[:, 0]) and np.all(opt.iterations > 0) and opt.attitude_peak.shape == (14, 4)
        # it is not the plain entry under another name, and the pieces add up at the result
        other = ctx.spacetime_lbfgs_host(3, so, b["waypoints"], b["times"], b["bc"], m, limits=lim, clearance=clr, **par)
        assert np.all(opt.objective[:, 0] > other[4][:, 0])
        peak = opt.attitude_peak.copy()
        f = opt.getCost() + 50.0 * np.add.reduceat(opt.getTimeAllocation(), so[:-1]) + opt.getFlightPenalty(m, limits=lim, clearance=clr) \
            + opt.getAttitudePenalty(**AO.ATTITUDE)
        assert np.max(np.abs(f - opt.objective[:, 1]) / opt.objective[:, 1]) <= 1e-9 and opt.attitude_peak.tobytes() == peak.tobytes()
        coef = opt.getPolyCoeff()
        assert opt.solve() is True and np.array_equal(opt.getPolyCoeff(), coef)
        with pytest.raises(ValueError):
            opt.optimizeTrajectoryAttitude(m, no_such_field=1.0)
        with pytest.raises(ValueError):
            opt.optimizeTrajectoryAttitude(m, attitude=dict(no_such_field=1.0))
        opt.setCorridor(b["waypoints"] - 0.1, b["waypoints"] + 0.1)
        with pytest.raises(ValueError):
            opt.optimizeTrajectoryAttitude(m)


def test_cpp_facade_optimize_trajectory_attitude(tmp_path):
    """TrajOptimizer::optimizeTrajectoryAttitude and getAttitudePenalty agree with the C ABI on the ragged batch."""
    r = 3
    b, sc = AO.batch_of(r, "ragged"), R.scene()
    so = np.ascontiguousarray(b["seg_offsets"], dtype=np.int32)
    n, total = so.size - 1, int(so[-1])
    idx = np.argwhere(sc["occ"] != 0)
    centres = np.asarray(W.ORIGIN) + (idx + 0.5) * W.RES
    lim, clr, att = R.LIMITS_OF[r], R.CLEARANCE, AO.ATTITUDE
    path = tmp_path / "ragged_batch.bin"
    with open(path, "wb") as fh:
        fh.write(np.array([r, n, total, len(centres), *W.DIMS, lim["samples_per_seg"], clr["samples_per_seg"], att["samples_per_seg"]],
                          dtype=np.int32).tobytes())
        fh.write(np.array([*W.ORIGIN, W.RES, W.MAX_DIST, lim["v_max"], lim["a_max"], lim["weight_v"], lim["weight_a"], clr["d_safe"], clr["weight"],
                           MOVE, att["gravity"], att["f_min"], att["f_max"], att["tilt_max"], att["rate_max"], att["weight_thrust"],
                           att["weight_tilt"], att["weight_rate"]], dtype=np.float64).tobytes())
        fh.write(so.tobytes())
        for key in ("waypoints", "times", "bc"):
            fh.write(np.ascontiguousarray(b[key], dtype=np.float64).tobytes())
        fh.write(np.ascontiguousarray(centres, dtype=np.float64).tobytes())
    rocm = "/opt/rocm"
    exe = os.path.join(ROOT, "tests", "cpp", "test_attitude_opt_facade")
    pkg = os.path.join(ROOT, "uav_motion_planning_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-I", os.path.join(rocm, "include"), f"-I{pkg}/cpp",
                           os.path.join(ROOT, "tests", "cpp", "test_attitude_opt_facade.cpp"), f"-L{pkg}", "-luavqp", f"-Wl,-rpath,{pkg}",
                           f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib", "-o", exe])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "optimizeTrajectoryAttitude: 14 trajectories" in out.stdout
