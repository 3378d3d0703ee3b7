"""-m gpu: the fused flight penalty and the joint waypoint / duration optimiser (uavqp_flight_penalty_*, uavqp_spacetime_optimize_*) against
the designed reference of tests/spacetime_reference.py: the oracle's exact solve, the longdouble penalties of
tests/limit_penalty_reference.py and tests/esdf_reference.py, scipy's L-BFGS-B.

Scene and cases (built once, in the reference modules): 32 x 32 x 16 voxels of 0.25 m with a pillar and a slab; the ragged batch of 14
trajectories (M = 2 .. 6 twice, 11, 1, 3, 5) plus one invalid trajectory, the uniform batch of 8 x 4 segments, and 4 x 11 segments; r = 3 and
4.  max_move = 1 m keeps every sample inside the map.  Limits and seeds: the rules in the docstring of tests/spacetime_reference.py.

Bounds.  Fused penalty (reference and device read the SAME device coefficients): 1e-9 of the per-trajectory largest magnitude of each output,
the tolerance of tests/test_gpu_limit_penalty.py and tests/test_gpu_esdf.py; the same against the sum of the two existing device entries.
Objective at the start and at the returned point against the reference's f there: 1e-9 relative; min_dist: 1e-9 x max(|reference|, one
voxel); peaks 1e-9 relative (the bounds of tests/test_gpu_waypoint_opt.py).  Against scipy: gap = (f_lib - f_scipy) / (f_start - f_scipy) <=
min(2 x R.GAP_AT_DEFAULT, 0.10); f_scipy per trajectory is the recorded result tests/golden/spacetime_scipy.json
(tools/spacetime_convergence.py --write-golden; tests/test_spacetime_contract.py recomputes one record and checks the rest of the file).  Everything else is exact.

Measured on MI355X: docs/measurement_log.md, "Joint optimisation of waypoints and durations"."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import uav_motion_planning_amd as U
from uav_motion_planning_amd import _lib
from uav_motion_planning_amd.esdf import EsdfMap

import esdf_reference as E
import limit_penalty_reference as L
import spacetime_reference as R
import waypoint_opt_reference as W

pytestmark = pytest.mark.gpu
LD = np.longdouble
PARITY = 1e-9
MOVE = R.PARAMS["max_move"]
GAP_BOUND = min(2.0 * R.GAP_AT_DEFAULT, 0.10)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spacetime_scipy.json")
OUT_KEYS = ("wp", "T", "coeff", "status", "obj", "acc", "peak", "md", "outside")


def defaults():
    p = _lib.SpacetimeParams()
    _lib.lib().uavqp_default_spacetime_params(ctypes.byref(p))
    return p


@pytest.fixture(scope="module")
def esdf(gpu_ctx):
    sc = R.scene()
    m = EsdfMap(gpu_ctx, W.DIMS, W.ORIGIN, W.RES, W.MAX_DIST)
    m.set_occupancy(sc["occ"])
    m.update()
    gpu_ctx.synchronize()
    yield m
    m.close()


def with_invalid(b):
    """The batch with one more trajectory in front of the last: a copy of trajectory 1 whose first duration is not positive."""
    so = b["seg_offsets"]
    wp, T, bc = R.split(b, 1)
    T = T.copy()
    T[0] = -1.0
    n = so.size - 1
    cut_s, cut_w = int(so[n - 1]), int(so[n - 1]) + n - 1
    Ms = np.concatenate([np.diff(so)[:n - 1], [T.size], np.diff(so)[n - 1:]])
    so2 = np.zeros(n + 2, dtype=np.int32)
    so2[1:] = np.cumsum(Ms)
    return dict(r=b["r"], seg_offsets=so2, waypoints=np.vstack([b["waypoints"][:cut_w], wp, b["waypoints"][cut_w:]]),
                times=np.concatenate([b["times"][:cut_s], T, b["times"][cut_s:]]),
                bc=np.concatenate([b["bc"][:n - 1], bc[None], b["bc"][n - 1:]])), n - 1


class Dev:
    """One batch on the device, through the device-pointer entries."""

    def __init__(self, ctx, b, uniform):
        import torch
        self.torch, self.ctx, self.b = torch, ctx, b
        self.r = b["r"]
        self.so = np.ascontiguousarray(b["seg_offsets"], dtype=np.int32)
        self.n, self.total = self.so.size - 1, int(self.so[-1])
        self.mmax = int(np.max(np.diff(self.so)))
        self.uni = self.mmax if uniform else 0
        self.dev = torch.device("cuda", 0)
        self.wp0 = np.ascontiguousarray(b["waypoints"], dtype=np.float64).reshape(-1, 3)
        self.T0 = np.ascontiguousarray(b["times"], dtype=np.float64).ravel()
        self.bc0 = np.ascontiguousarray(b["bc"], dtype=np.float64)
        self.d_so = self.up(self.so)
        self.d_bc = self.up(self.bc0)
        self.seg_traj = np.repeat(np.arange(self.n), np.diff(self.so))     # trajectory of every segment

    def up(self, x):
        return self.torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)

    def zeros(self, shape, dtype=None):
        return self.torch.zeros(shape, dtype=dtype or self.torch.float64, device=self.dev)

    def solve(self, d_wp, d_T):
        coeff, status = self.zeros(3 * 2 * self.r * self.total), self.zeros(self.n, self.torch.int32)
        self.torch.cuda.synchronize()
        self.ctx.solve_batch_device(self.r, self.n, self.uni, self.mmax, self.d_so, d_wp, d_T, self.d_bc, coeff, status)
        self.ctx.synchronize()
        return coeff, status

    def buffers(self):
        """Outputs of a penalty, pre-filled with NaN / -1: every element has to be written."""
        t = self.torch
        nan = lambda shape: self.zeros(shape) + math.nan
        return dict(phi=nan(self.n), grad_coeff=nan(3 * 2 * self.r * self.total), grad_times=nan(self.total), peak=nan((self.n, 2)),
                    min_dist=nan(self.n), outside=self.zeros(self.n, t.int32) - 1)

    def flight(self, esdf, d_T, coeff, status, want=None, limits=None, clearance=None):
        o = self.buffers()
        if want is not None:
            o = {k: (v if k in want else None) for k, v in o.items()}
        self.torch.cuda.synchronize()
        self.ctx.flight_penalty_device(self.r, self.n, self.uni, self.d_so, d_T, coeff, esdf, status=status, penalty=o["phi"],
                                       grad_coeff=o["grad_coeff"], grad_times=o["grad_times"], peak=o["peak"], min_dist=o["min_dist"],
                                       outside=o["outside"], limits=dict(R.LIMITS_OF[self.r], **(limits or {})), clearance=dict(R.CLEARANCE, **(clearance or {})))
        self.ctx.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}

    def separate(self, esdf, d_T, coeff, status, limits=None, clearance=None):
        """The two existing entries: (limit outputs, clearance outputs)."""
        a, b = self.buffers(), self.buffers()
        self.torch.cuda.synchronize()
        self.ctx.limit_penalty_device(self.r, self.n, self.uni, self.d_so, d_T, coeff, status=status, penalty=a["phi"], grad_coeff=a["grad_coeff"],
                                      grad_times=a["grad_times"], peak=a["peak"], **dict(R.LIMITS_OF[self.r], **(limits or {})))
        self.ctx.clearance_penalty_device(self.r, self.n, self.uni, self.d_so, d_T, coeff, esdf, status=status, penalty=b["phi"],
                                          grad_coeff=b["grad_coeff"], grad_times=b["grad_times"], min_dist=b["min_dist"], outside=b["outside"],
                                          **dict(R.CLEARANCE, **(clearance or {})))
        self.ctx.synchronize()
        return {k: v.cpu().numpy() for k, v in a.items()}, {k: v.cpu().numpy() for k, v in b.items()}

    def optimize(self, esdf, wp=None, T=None, limits=None, clearance=None, total=None, so=True, null=(), **params):
        t = self.torch
        d_wp, d_T = self.up(self.wp0 if wp is None else wp), self.up(self.T0 if T is None else T)
        out = dict(coeff=self.zeros(3 * 2 * self.r * self.total), status=self.zeros(self.n, t.int32), obj=self.zeros((self.n, 2)),
                   acc=self.zeros(self.n, t.int32), peak=self.zeros((self.n, 2)), md=self.zeros(self.n), outside=self.zeros(self.n, t.int32))
        params.setdefault("max_move", MOVE)
        arg = {k: (None if k in null else v) for k, v in out.items()}
        t.cuda.synchronize()
        self.ctx.spacetime_optimize_device(self.r, self.n, self.uni, self.mmax, self.total if total is None else total,
                                           self.d_so if so else None, d_wp, d_T, self.d_bc, esdf, arg["coeff"], arg["status"], arg["obj"],
                                           arg["acc"], arg["peak"], arg["md"], arg["outside"], limits=dict(R.LIMITS_OF[self.r], **(limits or {})),
                                           clearance=dict(R.CLEARANCE, **(clearance or {})), **params)
        self.ctx.synchronize()
        res = {k: v.cpu().numpy() for k, v in out.items()}
        res["wp"], res["T"] = d_wp.cpu().numpy(), d_T.cpu().numpy()
        res["d_wp"], res["d_T"] = d_wp, d_T
        res["bc"] = self.d_bc.cpu().numpy()
        return res


def make(gpu_ctx, r, kind):
    """-> (Dev, index of the invalid trajectory or None)"""
    if kind == "ragged":
        b, bad = with_invalid(R.cases(r))
        return Dev(gpu_ctx, b, False), bad
    return Dev(gpu_ctx, R.batch_of(r, kind), True), None


_runs = {}


def run_of(gpu_ctx, esdf, r, kind):
    """The default-parameter run of one of the three batches (computed once per module): (Dev, result, index of the invalid trajectory)."""
    key = (r, kind)
    if key not in _runs:
        d, bad = make(gpu_ctx, r, kind)
        _runs[key] = (d, d.optimize(esdf), bad)
    return _runs[key]


def valid_ids(d, bad):
    return [t for t in range(d.n) if t != bad]


def original_index(t, bad):
    """index in R.cases(r) of trajectory t of with_invalid(R.cases(r))"""
    return t if bad is None or t < bad else t - 1


def problem_of(oracle, r, kind, t):
    wp, T, bc = R.split(R.batch_of(r, kind), t)
    return R.Problem(oracle, r, wp, T, bc)


KINDS = [(3, "ragged"), (4, "ragged"), (3, "uniform"), (4, "uniform"), (3, "uniform11"), (4, "uniform11")]
IDS = [f"r{r}-{k}" for r, k in KINDS]
SCIPY_KINDS = KINDS[:4]
SCIPY_IDS = IDS[:4]


# ---------------------------------------------------------------------------------------------------
# uavqp_flight_penalty_*
# ---------------------------------------------------------------------------------------------------
def penalty_point(gpu_ctx, r, kind):
    """A solved point where both penalties are active: the start waypoints at 0.6 x the start durations."""
    d, bad = make(gpu_ctx, r, kind)
    T = np.where(d.T0 > 0, 0.6 * d.T0, d.T0)
    d_T = d.up(T)
    coeff, status = d.solve(d.up(d.wp0), d_T)
    st = status.cpu().numpy()
    assert np.all(st[valid_ids(d, bad)] == U.UAVQP_SOLVED) and (bad is None or st[bad] == U.UAVQP_INVALID_INPUT)
    return d, bad, T, d_T, coeff, status


def worst_errors(d, got, ref, keys):
    """max |got - ref| relative to the per-trajectory largest magnitude of ref, per output"""
    nc3 = 3 * 2 * d.r
    worst = {}
    for t in range(d.n):
        s0, s1 = int(d.so[t]), int(d.so[t + 1])
        sl = dict(phi=slice(t, t + 1), grad_coeff=slice(nc3 * s0, nc3 * s1), grad_times=slice(s0, s1), peak=t, min_dist=slice(t, t + 1))
        for key in keys:
            want = np.atleast_1d(ref[key][sl[key]]).astype(LD)
            have = np.atleast_1d(got[key][sl[key]]).astype(LD)
            scale = np.max(np.abs(want))
            err = float(np.max(np.abs(have - want)) / scale) if scale > 0 else float(np.max(np.abs(have)))
            worst[key] = max(worst.get(key, 0.0), err)
    return worst


@pytest.mark.parametrize("r,kind", KINDS, ids=IDS)
def test_flight_penalty_against_the_references_and_the_two_entries(gpu_ctx, esdf, r, kind):
    d, bad, T, d_T, coeff, status = penalty_point(gpu_ctx, r, kind)
    sc = R.scene()
    c, st = coeff.cpu().numpy(), status.cpu().numpy()
    lim = L.penalty(r, d.so, T, c, status=st, solved_value=U.UAVQP_SOLVED, **R.LIMITS_OF[r])
    clr = E.penalty(r, d.so, T, c, sc["dist"], sc["origin"], sc["res"], sc["max_dist"], status=st, solved_value=U.UAVQP_SOLVED, **R.CLEARANCE)
    ok = valid_ids(d, bad)
    # the case is worth comparing, and no sample sits on a discontinuity of the gradients
    assert np.count_nonzero(lim["phi"] > 0) * 2 >= d.n and np.count_nonzero(clr["phi"] > 0) * 2 >= d.n
    assert clr["margin"] >= 1e-6 and clr["gap"] >= 1e-9, (float(clr["margin"]), float(clr["gap"]))
    ref = dict(phi=lim["phi"] + clr["phi"], grad_coeff=lim["grad_coeff"] + clr["grad_coeff"], grad_times=lim["grad_times"] + clr["grad_times"],
               peak=lim["peak"], min_dist=clr["min_dist"])
    got = d.flight(esdf, d_T, coeff, status)
    keys = ("phi", "grad_coeff", "grad_times", "peak", "min_dist")
    worst = worst_errors(d, got, ref, keys)
    print(f"r={r} {kind}: fused penalty against the longdouble references, max error relative to the per-trajectory largest magnitude: "
          + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert np.array_equal(got["outside"].astype(np.int64), clr["outside"])
    for k, v in worst.items():
        assert v <= PARITY, f"{k}: {v:.3e}"
    # against the sum of the two existing device entries
    a, b = d.separate(esdf, d_T, coeff, status)
    both = dict(phi=a["phi"] + b["phi"], grad_coeff=a["grad_coeff"] + b["grad_coeff"], grad_times=a["grad_times"] + b["grad_times"],
                peak=a["peak"], min_dist=b["min_dist"])
    worst2 = worst_errors(d, got, both, keys)
    print(f"r={r} {kind}: against the sum of the two device entries: " + ", ".join(f"{k} {v:.3e}" for k, v in worst2.items()))
    assert np.array_equal(got["outside"], b["outside"])
    for k, v in worst2.items():
        assert v <= PARITY, f"{k}: {v:.3e}"
    # weights zeroed on one side reproduce the other entry alone
    only_clr = d.flight(esdf, d_T, coeff, status, limits=dict(weight_v=0.0, weight_a=0.0))
    for k, v in worst_errors(d, only_clr, dict(b, peak=a["peak"]), keys).items():
        assert v <= PARITY, f"limit weights zero, {k}: {v:.3e}"
    only_lim = d.flight(esdf, d_T, coeff, status, clearance=dict(weight=0.0))
    for k, v in worst_errors(d, only_lim, dict(a, min_dist=b["min_dist"]), keys).items():
        assert v <= PARITY, f"clearance weight zero, {k}: {v:.3e}"
    assert np.array_equal(only_clr["outside"], b["outside"]) and np.array_equal(only_lim["outside"], b["outside"])
    # the invalid trajectory: zeros of exactly zero bytes, min_dist = max_dist (the buffers were pre-filled with NaN / -1)
    if bad is not None:
        nc3, s0, s1 = 3 * 2 * r, int(d.so[bad]), int(d.so[bad + 1])
        assert got["phi"][bad:bad + 1].tobytes() == bytes(8) and got["peak"][bad].tobytes() == bytes(16)
        assert got["grad_coeff"][nc3 * s0:nc3 * s1].tobytes() == bytes(8 * nc3 * (s1 - s0)) and got["grad_times"][s0:s1].tobytes() == bytes(8 * (s1 - s0))
        assert got["min_dist"][bad] == W.MAX_DIST and got["outside"][bad] == 0
    assert not np.any(np.isnan(got["grad_coeff"])) and not np.any(np.isnan(got["grad_times"])) and np.all(got["outside"] >= 0)
    assert len(ok) >= 4


@pytest.mark.parametrize("r,kind", [(3, "ragged"), (4, "uniform")], ids=["r3-ragged", "r4-uniform"])
def test_flight_penalty_bytes_null_outputs_host_entry_and_arguments(gpu_ctx, esdf, r, kind):
    d, bad, T, d_T, coeff, status = penalty_point(gpu_ctx, r, kind)
    full = d.flight(esdf, d_T, coeff, status)
    again = d.flight(esdf, d_T, coeff, status)
    for k in full:
        assert full[k].tobytes() == again[k].tobytes(), k
    # samples per segment differ between the parts: each keeps its own
    mixed = d.flight(esdf, d_T, coeff, status, limits=dict(samples_per_seg=5), clearance=dict(samples_per_seg=11))
    a, b = d.separate(esdf, d_T, coeff, status, limits=dict(samples_per_seg=5), clearance=dict(samples_per_seg=11))
    both = dict(phi=a["phi"] + b["phi"], grad_coeff=a["grad_coeff"] + b["grad_coeff"], grad_times=a["grad_times"] + b["grad_times"],
                peak=a["peak"], min_dist=b["min_dist"])
    for k, v in worst_errors(d, mixed, both, ("phi", "grad_coeff", "grad_times", "peak", "min_dist")).items():
        assert v <= PARITY, f"K = 5 / 11, {k}: {v:.3e}"
    assert np.array_equal(mixed["outside"], b["outside"])
    # NULL outputs are honoured: every subset gives the same bytes for what it does return; all NULL is UAVQP_OK
    for want in (("phi",), ("grad_coeff",), ("grad_times", "outside"), ("peak",), ("min_dist",), ("phi", "grad_coeff", "grad_times")):
        part = d.flight(esdf, d_T, coeff, status, want=want)
        for k, v in part.items():
            assert (v is None) == (k not in want)
            if v is not None:
                assert v.tobytes() == full[k].tobytes(), (want, k)
    gpu_ctx.flight_penalty_device(r, d.n, d.uni, d.d_so, d_T, coeff, esdf)
    # the host entry
    host = gpu_ctx.flight_penalty_host(r, d.so, T, coeff.cpu().numpy(), esdf, uniform_segments=d.uni, status=status.cpu().numpy(),
                                       limits=R.LIMITS_OF[r], clearance=R.CLEARANCE)
    for k, v in zip(("phi", "grad_coeff", "grad_times", "peak", "min_dist", "outside"), host):
        assert v.tobytes() == full[k].tobytes(), k
    # invalid arguments
    phi = d.zeros(d.n)
    for bad_kw in (dict(limits=dict(v_max=0.0)), dict(limits=dict(weight_a=-1.0)), dict(limits=dict(samples_per_seg=0)),
                   dict(limits=dict(a_max=math.inf)), dict(clearance=dict(d_safe=0.0)), dict(clearance=dict(weight=math.nan)),
                   dict(clearance=dict(samples_per_seg=0))):
        with pytest.raises(U.UavqpError):
            gpu_ctx.flight_penalty_device(r, d.n, d.uni, d.d_so, d_T, coeff, esdf, penalty=phi, **bad_kw)
    with pytest.raises(U.UavqpError):
        gpu_ctx.flight_penalty_device(5, d.n, d.uni, d.d_so, d_T, coeff, esdf, penalty=phi)
    with pytest.raises(U.UavqpError):
        gpu_ctx.flight_penalty_device(r, d.n, d.uni, d.d_so, d_T, coeff, None, penalty=phi)              # a NULL map
    with pytest.raises(U.UavqpError):
        gpu_ctx.flight_penalty_device(r, d.n, d.uni, d.d_so, None, coeff, esdf, penalty=phi)              # NULL times
    with pytest.raises(U.UavqpError):
        gpu_ctx.flight_penalty_device(r, d.n, 0, None, d_T, coeff, esdf, penalty=phi)                     # ragged without offsets
    fresh = EsdfMap(gpu_ctx, (4, 4, 4), (0.0, 0.0, 0.0), 0.5)
    with pytest.raises(U.UavqpError):
        gpu_ctx.flight_penalty_device(r, d.n, d.uni, d.d_so, d_T, coeff, fresh, penalty=phi)              # a map that was never updated
    fresh.close()


def test_torch_flight_penalty_equals_the_c_abi_byte_for_byte(gpu_ctx, esdf):
    from uav_motion_planning_amd import autograd
    d, bad, T, d_T, coeff, status = penalty_point(gpu_ctx, 3, "uniform")
    full = d.flight(esdf, d_T, coeff, status)
    c, t = coeff.clone().requires_grad_(True), d_T.clone().requires_grad_(True)
    out = autograd.flight_penalty(gpu_ctx, 3, c, t, esdf, uniform_segments=d.uni, status=status, limits=R.LIMITS_OF[3], clearance=R.CLEARANCE)
    out.sum().backward()
    assert out.detach().cpu().numpy().tobytes() == full["phi"].tobytes()
    assert c.grad.cpu().numpy().tobytes() == full["grad_coeff"].tobytes() and t.grad.cpu().numpy().tobytes() == full["grad_times"].tobytes()


# ---------------------------------------------------------------------------------------------------
# uavqp_spacetime_optimize_*: invariants, all exact
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,kind", KINDS, ids=IDS)
def test_optimiser_invariants(gpu_ctx, esdf, r, kind):
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    P = defaults()
    ok = valid_ids(d, bad)
    st = res["status"]
    assert np.all(st[ok] == U.UAVQP_SOLVED)
    assert np.all(res["obj"][ok, 1] <= res["obj"][ok, 0])
    assert np.all(res["acc"] >= 0) and np.all(res["acc"] <= P.max_iters)
    assert np.array_equal(res["bc"], d.bc0)
    lo, hi = d.wp0 - MOVE, d.wp0 + MOVE
    assert np.all(res["wp"] >= lo) and np.all(res["wp"] <= hi)
    seg_ok = d.seg_traj != (-1 if bad is None else bad)
    assert np.all(res["T"][seg_ok] >= P.t_min) and np.all(res["T"][seg_ok] <= P.t_max)
    for t in range(d.n):
        k0, k1 = int(d.so[t]) + t, int(d.so[t + 1]) + t
        s0, s1 = int(d.so[t]), int(d.so[t + 1])
        assert res["wp"][[k0, k1]].tobytes() == d.wp0[[k0, k1]].tobytes(), "an end knot moved"
        if t == bad:
            assert st[t] == U.UAVQP_INVALID_INPUT
            assert res["wp"][k0:k1 + 1].tobytes() == d.wp0[k0:k1 + 1].tobytes() and res["T"][s0:s1].tobytes() == d.T0[s0:s1].tobytes()
            assert np.all(np.isnan(res["obj"][t])) and res["acc"][t] == 0
        else:
            assert res["acc"][t] > 0 and res["obj"][t, 1] < res["obj"][t, 0], f"trajectory {t} was left out"
            assert np.any(res["T"][s0:s1] != d.T0[s0:s1])
            if s1 - s0 == 1:
                assert res["wp"][k0:k1 + 1].tobytes() == d.wp0[k0:k1 + 1].tobytes(), "the M = 1 trajectory changes only its duration"
            else:
                assert np.any(res["wp"][k0:k1 + 1] != d.wp0[k0:k1 + 1])
    # the coefficients and the status are a plain solve at the point handed back
    fresh, st2 = d.solve(res["d_wp"], res["d_T"])
    assert fresh.cpu().numpy().tobytes() == res["coeff"].tobytes() and np.array_equal(st2.cpu().numpy(), st)
    # the diagnostics are the fused penalty's at the point handed back
    pen = d.flight(esdf, res["d_T"], fresh, st2, want=("peak", "min_dist", "outside"))
    assert pen["peak"].tobytes() == res["peak"].tobytes() and pen["min_dist"].tobytes() == res["md"].tobytes()
    assert np.array_equal(pen["outside"], res["outside"])
    # run to run: identical bytes (NaN objectives of the invalid trajectory compared as bytes too)
    again = d.optimize(esdf)
    for k in OUT_KEYS:
        assert res[k].tobytes() == again[k].tobytes(), k
    print(f"r={r} {kind}: median f_result / f_start {np.median(res['obj'][ok, 1] / res['obj'][ok, 0]):.4f}, accepted min / median / max "
          f"{res['acc'][ok].min()} / {int(np.median(res['acc'][ok]))} / {res['acc'][ok].max()} of {P.max_iters}, sum T "
          f"{d.T0[seg_ok].sum():.2f} -> {res['T'][seg_ok].sum():.2f}")


@pytest.mark.parametrize("r", [3, 4])
def test_uniform_call_equals_ragged_call(gpu_ctx, esdf, r):
    """Eleven segments: no specialised solve kernel, so both calls run the same solve and every byte must agree."""
    d, res, _ = run_of(gpu_ctx, esdf, r, "uniform11")
    other = Dev(gpu_ctx, d.b, False).optimize(esdf)
    for k in OUT_KEYS:
        assert res[k].tobytes() == other[k].tobytes(), k


@pytest.mark.parametrize("r,kind", [(3, "ragged"), (4, "uniform")], ids=["r3-ragged", "r4-uniform"])
def test_host_entry_equals_device_entry(gpu_ctx, esdf, r, kind):
    d, res, _ = run_of(gpu_ctx, esdf, r, kind)
    got = gpu_ctx.spacetime_optimize_host(r, d.so, d.wp0, d.T0, d.bc0, esdf, uniform_segments=d.uni, limits=R.LIMITS_OF[r], clearance=R.CLEARANCE,
                                          max_move=MOVE)
    # (the coefficients of the invalid trajectory: the host entry hands back zeros, the device entry leaves the test's zeroed buffer alone)
    for k, v in zip(OUT_KEYS, got):
        assert res[k].tobytes() == v.tobytes(), k


@pytest.mark.parametrize("r,kind", [(3, "ragged"), (4, "uniform")], ids=["r3-ragged", "r4-uniform"])
def test_max_iters_zero_is_the_plain_solve_after_the_projection(gpu_ctx, esdf, r, kind):
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    ok = valid_ids(d, bad)
    seg_ok = d.seg_traj != (-1 if bad is None else bad)
    t_min, t_max = 1.05 * d.T0[seg_ok].min(), 0.95 * d.T0[seg_ok].max()     # both bounds bind somewhere
    z = d.optimize(esdf, max_iters=0, t_min=t_min, t_max=t_max)
    T_want = np.where(seg_ok, np.minimum(np.maximum(d.T0, t_min), t_max), d.T0)
    assert z["wp"].tobytes() == d.wp0.tobytes() and z["T"].tobytes() == T_want.tobytes()
    assert np.any(T_want != d.T0)
    plain, st_plain = d.solve(d.up(d.wp0), d.up(T_want))
    assert z["coeff"].tobytes() == plain.cpu().numpy().tobytes() and np.array_equal(z["status"], st_plain.cpu().numpy())
    assert np.array_equal(z["obj"][ok, 0], z["obj"][ok, 1]) and np.all(z["acc"] == 0)
    pen = d.flight(esdf, d.up(T_want), plain, st_plain, want=("peak", "min_dist", "outside"))
    assert pen["peak"].tobytes() == z["peak"].tobytes() and pen["min_dist"].tobytes() == z["md"].tobytes() and np.array_equal(pen["outside"], z["outside"])
    # without binding bounds the start objective is that of the default run
    z2 = d.optimize(esdf, max_iters=0)
    assert z2["T"].tobytes() == d.T0.tobytes() and np.array_equal(z2["obj"][ok, 0], res["obj"][ok, 0])


def test_optional_outputs_may_be_null(gpu_ctx, esdf):
    d, res, _ = run_of(gpu_ctx, esdf, 4, "uniform")
    part = d.optimize(esdf, null=("status", "acc", "peak", "md", "outside"))
    for k in ("wp", "T", "coeff", "obj"):
        assert part[k].tobytes() == res[k].tobytes(), k
    part = d.optimize(esdf, null=("peak", "outside"))
    for k in ("wp", "T", "coeff", "obj", "status", "acc", "md"):
        assert part[k].tobytes() == res[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------
# against the reference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,kind", SCIPY_KINDS, ids=SCIPY_IDS)
def test_objective_and_diagnostics_vs_reference(gpu_ctx, esdf, oracle, r, kind):
    """f, the peaks, min_dist and outside at the start and at the returned point: the oracle's solve + the longdouble penalties."""
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    start = d.optimize(esdf, max_iters=0)
    worst_f, worst_d, worst_p = 0.0, 0.0, 0.0
    for t in valid_ids(d, bad):
        prob = problem_of(oracle, r, kind, original_index(t, bad))
        k0, k1, s0, s1 = int(d.so[t]) + t, int(d.so[t + 1]) + t, int(d.so[t]), int(d.so[t + 1])
        for got, q in ((start, prob.parts(prob.start_p, R.clamp_times(prob.start_T))), (res, prob.parts(res["wp"][k0:k1 + 1], res["T"][s0:s1]))):
            col = 0 if got is start else 1
            worst_f = max(worst_f, abs(got["obj"][t, col] - q["f"]) / q["f"])
            worst_d = max(worst_d, abs(got["md"][t] - q["min_dist"]) / max(abs(q["min_dist"]), W.RES))
            worst_p = max(worst_p, float(np.max(np.abs(got["peak"][t] - q["peak"]) / q["peak"])))
            assert q["outside"] == 0 and got["outside"][t] == 0
    print(f"r={r} {kind}: max rel err vs reference: objective {worst_f:.3e}, min_dist {worst_d:.3e}, peaks {worst_p:.3e}")
    assert worst_f <= 1e-9
    assert worst_d <= 1e-9
    assert worst_p <= 1e-9


@pytest.mark.parametrize("r,kind", SCIPY_KINDS, ids=SCIPY_IDS)
def test_optimiser_vs_scipy_lbfgsb_on_the_reference(gpu_ctx, esdf, r, kind):
    d, res, bad = run_of(gpu_ctx, esdf, r, kind)
    P = defaults()
    golden = json.load(open(GOLDEN))[f"r{r}-{kind}"]
    worst, ratios, count = -math.inf, [], 0
    for t in valid_ids(d, bad):
        rec = golden[original_index(t, bad)]
        f_start, f_scipy = res["obj"][t, 0], rec["f_scipy"]
        assert abs(f_start - rec["f_start"]) <= 1e-9 * f_start, "the recorded results belong to other cases"
        assert rec["outside"] == 0
        assert f_start > 1.5 * f_scipy, "the case has no decrease to speak of"
        gap = (res["obj"][t, 1] - f_scipy) / (f_start - f_scipy)
        worst = max(worst, gap)
        ratios.append(f_start / f_scipy)
        count += 1
        assert gap <= GAP_BOUND, f"r={r} {kind} trajectory {t}: gap {gap:.3e}"
    print(f"r={r} {kind}: {count} trajectories, f_start / f_scipy {min(ratios):.1f} .. {max(ratios):.1f}, worst gap {worst:.3e} "
          f"at max_iters = {P.max_iters} (bound {GAP_BOUND:.4f})")
    assert count == d.n - (0 if bad is None else 1), "no trajectory is left out except the designed invalid one"


@pytest.mark.parametrize("r,kind", SCIPY_KINDS, ids=SCIPY_IDS)
def test_penalised_trajectories_end_slower_and_farther_away(gpu_ctx, esdf, r, kind):
    """Against a run with both limit weights zero: a lower peak in every component in which that run exceeds the limit, and at least half
    of the trajectories are compared.  Against a run with clearance weight zero: a larger smallest distance where that run comes closer
    than d_safe (one segment has no waypoint to move), at least half compared."""
    d, _, bad = run_of(gpu_ctx, esdf, r, kind)
    ok = [t for t in valid_ids(d, bad)]
    inner = np.array([int(d.so[t + 1] - d.so[t]) > 1 for t in ok])
    n = R.FEASIBILITY_ITERS     # all three runs at the trial count the seed rule was evaluated at on the CPU
    res = d.optimize(esdf, max_iters=n)
    nolim = d.optimize(esdf, max_iters=n, limits=dict(weight_v=0.0, weight_a=0.0))
    noclr = d.optimize(esdf, max_iters=n, clearance=dict(weight=0.0))
    over = nolim["peak"][ok] > 1.0
    assert np.count_nonzero(over.any(axis=1)) * 2 >= len(ok), "fewer than half of the trajectories exceed a limit without the penalty"
    assert np.all(res["peak"][ok][over] < nolim["peak"][ok][over])
    close = (noclr["md"][ok] < R.CLEARANCE["d_safe"]) & inner
    assert np.count_nonzero(close) * 2 >= len(ok)
    assert np.all(res["md"][ok][close] > noclr["md"][ok][close])
    assert np.all(res["outside"][ok] == 0) and np.all(nolim["outside"][ok] == 0) and np.all(noclr["outside"][ok] == 0)
    print(f"r={r} {kind}: {np.count_nonzero(over.any(axis=1))} of {len(ok)} exceed a limit without the limit penalty; worst peaks v / a "
          f"{nolim['peak'][ok].max(axis=0)} -> {res['peak'][ok].max(axis=0)}; {np.count_nonzero(close)} come closer than d_safe without the "
          f"clearance penalty, smallest distance {noclr['md'][ok].min():.3f} -> {res['md'][ok].min():.3f}")


# ---------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused(gpu_ctx, esdf):
    d = Dev(gpu_ctx, R.uniform_cases(3), True)
    rg = Dev(gpu_ctx, R.cases(3), False)
    inf, nan = math.inf, math.nan
    for bad in (dict(max_iters=-1), dict(smooth_weight=-1.0), dict(smooth_weight=inf), dict(smooth_weight=nan), dict(time_weight=0.0),
                dict(time_weight=-1.0), dict(time_weight=inf), dict(time_weight=nan), dict(t_min=0.0), dict(t_min=-1.0), dict(t_min=nan),
                dict(t_min=2.0, t_max=1.0), dict(t_max=inf), dict(t_max=nan), dict(max_move=0.0), dict(max_move=-1.0), dict(max_move=nan),
                dict(initial_step_move=0.0), dict(initial_step_move=inf), dict(initial_step_log=0.0), dict(initial_step_log=inf),
                dict(initial_step_log=nan), dict(armijo_c=0.0), dict(armijo_c=1.0), dict(shrink=0.0), dict(shrink=1.0), dict(grow=0.5),
                dict(grow=inf)):
        with pytest.raises(U.UavqpError):
            d.optimize(esdf, **bad)
    with pytest.raises(ValueError):
        d.optimize(esdf, struct_size=4)
    pp, cp, lp = defaults(), _lib.ClearanceParams(), _lib.LimitParams()
    _lib.lib().uavqp_default_clearance_params(ctypes.byref(cp))
    _lib.lib().uavqp_default_limit_params(ctypes.byref(lp))
    pp.struct_size = 4
    d_T = d.up(d.T0)
    args = (gpu_ctx._h, 3, d.n, d.uni, d.mmax, d.total, None, d.up(d.wp0).data_ptr(), d_T.data_ptr(), d.d_bc.data_ptr(), esdf.handle,
            ctypes.byref(lp), ctypes.byref(cp), ctypes.byref(pp), d.zeros(3 * 6 * d.total).data_ptr(), None, d.zeros((d.n, 2)).data_ptr(), None, None,
            None, None)
    assert _lib.lib().uavqp_spacetime_optimize_device(*args) == _lib.UAVQP_ERR_INVALID_ARG        # a wrong struct_size
    for bad in (dict(d_safe=0.0), dict(weight=-1.0), dict(samples_per_seg=0)):
        with pytest.raises(U.UavqpError):
            d.optimize(esdf, clearance=bad)
    for bad in (dict(v_max=0.0), dict(a_max=-1.0), dict(weight_v=-1.0), dict(weight_a=inf), dict(samples_per_seg=0)):
        with pytest.raises(U.UavqpError):
            d.optimize(esdf, limits=bad)
    with pytest.raises(U.UavqpError):
        d.optimize(None)                                               # a NULL map
    fresh = EsdfMap(gpu_ctx, (4, 4, 4), (0.0, 0.0, 0.0), 0.5)
    with pytest.raises(U.UavqpError):
        d.optimize(fresh)                                              # a map that was never updated
    fresh.close()
    with pytest.raises(U.UavqpError):
        rg.optimize(esdf, so=False)                                    # ragged without offsets
    with pytest.raises(U.UavqpError):
        d.optimize(esdf, total=d.total + 1)                            # a wrong total_segments
    with pytest.raises(U.UavqpError):
        d.optimize(esdf, null=("obj",))                                # objective_out is not optional
    # every bound that is allowed: max_move = INFINITY, t_min = t_max, smooth_weight = 0, grow = 1
    res = d.optimize(esdf, max_move=inf, max_iters=4, smooth_weight=0.0, grow=1.0)
    assert np.all(res["status"] == U.UAVQP_SOLVED) and np.all(res["obj"][:, 1] <= res["obj"][:, 0])
    res = d.optimize(esdf, max_iters=4, t_min=1.0, t_max=1.0)
    assert np.all(res["T"] == 1.0) and np.all(res["status"] == U.UAVQP_SOLVED)
