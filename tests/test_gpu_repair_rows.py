"""-m gpu: the rows repair of the corridor pipeline (include/uavqp.h uavqp_repair_rows_from_hits_device,
uavqp_corridor_pipeline_rows_device / _host, pipeline.corridor_pipeline_device(repair="rows"), TrajOptimizer::solvePipeline(...,
PipelineRepair::Rows)).  The kernel is held to the numpy restatement of tests/test_repair_rows_contract.py."""
import os

import numpy as np
import pytest

import uav_motion_planning_amd as U
from uav_motion_planning_amd import workloads as W
from test_repair_rows_contract import restate_rows_from_hits
from test_real_frontend_fixture import load_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _up(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _rows_state(S):
    return np.zeros((S, 2)), -np.ones((S, 2), dtype=np.int32), np.zeros((S, 2, 3)), np.zeros((S, 2, 3))


@pytest.mark.parametrize("r,uniform", [(3, 0), (4, 0), (3, 6), (4, 6)])
def test_rows_from_hits_kernel_matches_the_restatement(gpu_ctx, r, uniform):
    import torch
    n = 24
    b = W.uniform_batch(5, n, uniform, r) if uniform else W.ragged_batch(5, n, r, m_lo=2, m_hi=9)
    so = np.asarray(b["seg_offsets"], dtype=np.int32)
    S = int(so[-1])
    wp = np.asarray(b["waypoints"]).reshape(-1, 3)
    T = np.asarray(b["times"], dtype=np.float64).reshape(-1)
    coef, st = gpu_ctx.solve_batch_host(r, None if uniform else so, wp, T, b["bc"], uniform_segments=uniform)
    assert np.all(st == U.UAVQP_SOLVED)
    obs = W.pillar_cloud(5, n_pillars=40, resolution=0.25)
    ns = 64
    tot = np.array([T[so[k]:so[k + 1]].sum() for k in range(n)])
    dt = float(tot.max() / (ns - 1))
    rng = np.random.default_rng(7 + r + uniform)

    def flags_with_runs(lo_frac, hi_frac):
        fl = np.zeros((n, ns), dtype=np.uint8)
        for k in range(n):
            for _ in range(rng.integers(1, 5)):
                a = int(rng.integers(int(lo_frac * ns), int(hi_frac * ns)))
                fl[k, a:a + int(rng.integers(1, 6))] = 1
        return fl

    d = {k: _up(v) for k, v in dict(so=so, wp=wp, T=T, coef=coef, obs=obs).items()}
    state = _rows_state(S)
    g_state = [_up(x) for x in state]
    new = torch.zeros(n, dtype=torch.int32, device=g_state[0].device)
    fl1, fl2 = flags_with_runs(0.0, 0.6), flags_with_runs(0.3, 1.0)
    placed_total = 0
    for call, fl in enumerate((fl1, fl2, fl2)):
        ref = restate_rows_from_hits(r, so, T, coef, ns, 0.0, dt, fl, obs, 0.4, 0.1, 0.8, *state)
        gpu_ctx.repair_rows_from_hits_device(r, n, uniform, None if uniform else d["so"], d["wp"], d["T"], d["coef"], ns, 0.0, dt, _up(fl),
                                             d["obs"], obs.shape[0], 0.4, 0.1, 0.8, *g_state, new)
        gpu_ctx.synchronize()
        got = [x.cpu().numpy() for x in g_state]
        tie = ref[5]
        ok = ~tie
        assert np.array_equal(got[1][ok], ref[1][ok]), call
        assert np.array_equal(got[0][ok], ref[0][ok]), call
        used = ok[:, None] & (ref[1] >= 0)
        scale = np.maximum(1.0, np.abs(ref[2][used]))
        assert np.all(np.abs(got[2][used] - ref[2][used]) <= 1e-9 * scale), call
        assert np.all(np.abs(got[3][used] - ref[3][used]) <= 1e-9 * scale), call
        seg_owner = np.repeat(np.arange(n), np.diff(so))
        clean = np.ones(n, dtype=bool)
        clean[seg_owner[tie]] = False
        assert np.array_equal(new.cpu().numpy()[clean], ref[4][clean]), call
        if call == 0:
            assert ref[4].sum() > n // 2
        if call == 1:
            assert (got[1][:, 1] >= 0).sum() > 0          # slot 1 filled
        if call == 2:
            assert new.cpu().numpy().sum() == 0 and ref[4].sum() == 0
        placed_total += int(ref[4].sum())
        state = tuple(got)                               # the next call continues from the kernel's own state
    assert placed_total == int((state[1] >= 0).sum())


def _kino_batch(r):
    from uav_motion_planning_amd import adapters as A
    meta, paths, durs, v0 = load_fixture()
    b = A.flatten_paths(paths, durs)
    b["bc"] = A.boundary_from_odometry(len(paths), r, v0)
    m = meta["map"]
    cloud = W.pillar_cloud(m["config_index"], n_pillars=m["n_pillars"], resolution=m["resolution"])
    return b, cloud


def _run(r, b, cloud, repair, repair_rounds, **kw):
    from uav_motion_planning_amd.pipeline import corridor_pipeline_device
    so = np.asarray(b["seg_offsets"], dtype=np.int32)
    d_T = _up(np.asarray(b["times"], dtype=np.float64).copy())
    with U.Context(0) as ctx:
        res = corridor_pipeline_device(ctx, r, _up(so), _up(np.asarray(b["waypoints"]).reshape(-1, 3)), d_T, _up(b["bc"]), _up(cloud),
                                       int(np.diff(so).max()), repair_rounds=repair_rounds, repair=repair, **kw)
        out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in dict(res).items()}
    out["T"] = d_T.cpu().numpy()
    return out


def _snap_energy(c, T):
    """integral of |p''''|^2 over one segment, c [3, 8] ascending."""
    e = 0.0
    for ax in range(3):
        s = np.polyder(c[ax, ::-1], 4)
        e += np.polyval(np.polyint(np.polymul(s, s)), T)
    return e


def _eval(c, t, d=0):
    return np.array([np.polyval(np.polyder(c[ax, ::-1], d) if d else c[ax, ::-1], t) for ax in range(3)])


def test_kino_fixture_rows_repair(oracle):
    from oracle.certificates import kkt_certificate_rows
    r = 4
    b, cloud = _kino_batch(r)
    so = np.asarray(b["seg_offsets"])
    n = so.size - 1
    wp = np.asarray(b["waypoints"]).reshape(-1, 3)
    bc = np.asarray(b["bc"])
    z = _run(r, b, cloud, "boxes", 0)
    box = _run(r, b, cloud, "boxes", 2)
    rw = _run(r, b, cloud, "rows", 2)
    assert np.all(rw["status"] == U.UAVQP_SOLVED)
    n_after = int((~rw["collision_free"]).sum())
    print("kino fixture: colliding before repair %d, after box repair %d, after rows repair %d (rows kept %d, repairs %d)"
          % (rw["colliding_before_repair"], int((~box["collision_free"]).sum()), n_after, rw["repair_rows"], rw["repairs"]))
    assert rw["colliding_before_repair"] == z["colliding_before_repair"]
    assert n_after < rw["colliding_before_repair"] and rw["repair_rows"] > 0
    assert int((rw["row_deriv"] >= 0).sum()) == rw["repair_rows"]
    # knot boxes are never changed; a trajectory without a kept row is the repair_rounds = 0 output bit for bit
    assert np.array_equal(rw["corr_lo"], z["corr_lo"]) and np.array_equal(rw["corr_hi"], z["corr_hi"])
    has_row = np.array([(rw["row_deriv"][so[k]:so[k + 1]] >= 0).any() for k in range(n)])
    nc = 24
    ratios = []
    for k in range(n):
        sl, cs = slice(so[k], so[k + 1]), slice(nc * so[k], nc * so[k + 1])
        if not has_row[k]:
            assert np.array_equal(rw["coeff"][cs], z["coeff"][cs]) and np.array_equal(rw["T"][sl], z["T"][sl]) and rw["status"][k] == z["status"][k], k
            continue
        M = int(so[k + 1] - so[k])
        T = rw["T"][sl]
        c = rw["coeff"][cs].reshape(3, M, 8)
        rows = []
        for i in range(M):
            for j in range(2):
                sg = so[k] + i
                if rw["row_deriv"][sg, j] < 0:
                    continue
                tau = rw["row_tau"][sg, j]
                p = _eval(c[:, i], tau * T[i])
                lo, hi = rw["row_lo"][sg, j], rw["row_hi"][sg, j]
                assert np.all(p >= lo - 1e-9) and np.all(p <= hi + 1e-9), (k, i, j)
                rows.append((i, tau, lo, hi))
        for ax in range(3):
            prim, stat, comp = kkt_certificate_rows(r, M, T, c[ax].ravel(), wp[so[k] + k:so[k + 1] + k + 1, ax], bc[k, 0, :, ax], bc[k, 1, :, ax],
                                                    rw["corr_lo"][so[k] + k + 1:so[k + 1] + k, ax], rw["corr_hi"][so[k] + k + 1:so[k + 1] + k, ax],
                                                    [(i, tau, 0, lo[ax], hi[ax]) for (i, tau, lo, hi) in rows])
            assert prim < 1e-9 and stat < 1e-6 and comp < 1e-5, (k, ax, prim, stat, comp)
        Tb = box["T"][sl]
        cb = box["coeff"][cs].reshape(3, M, 8)
        e_rows = sum(_snap_energy(c[:, i], T[i]) for i in range(M))
        e_box = sum(_snap_energy(cb[:, i], Tb[i]) for i in range(M))
        ratios.append(e_rows / e_box)
    print("kino fixture: %d trajectories repaired with rows, median snap-energy ratio rows / boxes %.3f"
          % (len(ratios), float(np.median(ratios)) if ratios else float("nan")))


def test_rows_entry_without_repair_rounds_is_the_box_entry(oracle):
    r = 4
    b, cloud = _kino_batch(r)
    a = _run(r, b, cloud, "boxes", 0)
    c = _run(r, b, cloud, "rows", 0)
    for k in ("coeff", "status", "corr_lo", "corr_hi", "first_hit", "T"):
        assert np.array_equal(a[k], c[k]), k
    for k in ("colliding_before_repair", "colliding_with_blocked_waypoints", "repairs", "rounds", "still_stretching", "check_dt", "all_solved"):
        assert a[k] == c[k], k
    assert c["repair_rows"] == 0 and np.all(c["row_deriv"] == -1)


def test_config5_shaped_batch_with_an_enlarged_check(oracle):
    r, n = 4, 300
    b = W.ragged_batch(5, n, r, m_lo=3, m_hi=20)
    obs = W.pillar_cloud(5, n_pillars=50, resolution=0.25)
    kw = dict(check_robot=(0.6, 0.2))
    z = _run(r, b, obs, "boxes", 0, **kw)
    runs = [_run(r, b, obs, "rows", 2, **kw) for _ in range(2)]
    a = runs[0]
    print("config-5 batch, enlarged check: colliding %d -> %d, rows kept %d, repairs %d"
          % (a["colliding_before_repair"], int((~a["collision_free"]).sum()), a["repair_rows"], a["repairs"]))
    assert a["colliding_before_repair"] > 0 and a["repairs"] >= 1
    assert np.all((a["status"] == U.UAVQP_SOLVED) | (a["status"] == z["status"]))
    for k in ("coeff", "status", "T", "row_tau", "row_deriv", "row_lo", "row_hi", "first_hit"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    assert runs[0]["repair_rows"] == runs[1]["repair_rows"]


def test_cpp_solve_pipeline_with_rows_repair():
    """tests/cpp/test_pipeline_rows_repair.cpp: TrajOptimizer::solvePipeline(..., PipelineRepair::Rows) on a small ragged batch."""
    import shutil
    import subprocess
    rocm = "/opt/rocm"
    if shutil.which("g++") is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no g++ / HIP headers on this box")
    exe = os.path.join(ROOT, "tests", "cpp", "test_pipeline_rows_repair")
    libdir = os.path.join(ROOT, "uav_motion_planning_amd")
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(rocm, "include"), "-I", os.path.join(libdir, "cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_pipeline_rows_repair.cpp"), "-o", exe, "-L", libdir, "-luavqp",
           "-L", os.path.join(rocm, "lib"), "-lamdhip64", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{rocm}/lib"]
    cp = subprocess.run(cmd, capture_output=True, text=True)
    assert cp.returncode == 0, cp.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "OK" in run.stdout, run.stdout + run.stderr
