"""-m gpu: the facades of the joint optimiser with limited-memory BFGS directions -- Python TrajOptimizer.optimizeTrajectoryLbfgs and the C++
TrajOptimizer::optimizeTrajectoryLbfgs of cpp/traj_optimizer.h with the uavqp::EsdfMap of cpp/esdf_map.h
(tests/cpp/test_spacetime_lbfgs_facade.cpp, built and run the way tests/test_gpu_spacetime_facade.py does): both reproduce
uavqp_spacetime_lbfgs_host byte for byte on the ragged batch of tests/test_gpu_spacetime_lbfgs.py (r = 3, 14 trajectories)."""
import os
import subprocess

import numpy as np
import pytest

import uav_motion_planning_amd as U
from uav_motion_planning_amd.esdf import EsdfMap

import spacetime_reference as R
import waypoint_opt_reference as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_facade_optimize_trajectory_lbfgs():
    b = R.cases(3)
    so = b["seg_offsets"]
    lim, clr, par = dict(R.LIMITS_OF[3]), dict(R.CLEARANCE), dict(max_move=1.0, memory=4)
    opt = U.TrajOptimizer(order=3)
    opt.setWaypoints(b["waypoints"], wp_offsets=so + np.arange(so.size))
    opt.setTimeAllocation(b["times"])
    opt.setBoundary(b["bc"])
    ctx = opt.context()
    sc = R.scene()
    with EsdfMap(ctx, W.DIMS, W.ORIGIN, W.RES, W.MAX_DIST) as m:
        m.set_occupancy(sc["occ"])
        m.update()
        want = ctx.spacetime_lbfgs_host(3, so, b["waypoints"], b["times"], b["bc"], m, limits=lim, clearance=clr, **par)
        assert opt.optimizeTrajectoryLbfgs(m, limits=lim, clearance=clr, **par) is True
        got = (opt.getWaypoints(), opt.getTimeAllocation(), opt.getPolyCoeff(), opt.status, opt.objective, opt.iterations, opt.peak, opt.min_dist,
               opt.outside)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        assert np.all(opt.objective[:, 1] < opt.objective[:, 0]) and np.all(opt.outside == 0) and np.all(opt.iterations > 0)
        # it is not the projected-gradient entry under another name
        other = ctx.spacetime_optimize_host(3, so, b["waypoints"], b["times"], b["bc"], m, limits=lim, clearance=clr, max_move=1.0)
        assert other[4][:, 0].tobytes() == opt.objective[:, 0].tobytes() and np.all(opt.objective[:, 1] != other[4][:, 1])
        # getPolyCoeff stays valid: it is the solve at the stored waypoints and durations
        coef = opt.getPolyCoeff()
        assert opt.solve() is True and np.array_equal(opt.getPolyCoeff(), coef)
        with pytest.raises(ValueError):
            opt.optimizeTrajectoryLbfgs(m, no_such_field=1.0)
        opt.setCorridor(b["waypoints"] - 0.1, b["waypoints"] + 0.1)
        with pytest.raises(ValueError):
            opt.optimizeTrajectoryLbfgs(m)


def test_cpp_facade_optimize_trajectory_lbfgs(tmp_path):
    """TrajOptimizer::optimizeTrajectoryLbfgs agrees with the C ABI on the ragged batch."""
    r = 3
    b, sc = R.cases(r), R.scene()
    so = np.ascontiguousarray(b["seg_offsets"], dtype=np.int32)
    n, total = so.size - 1, int(so[-1])
    idx = np.argwhere(sc["occ"] != 0)
    centres = np.asarray(W.ORIGIN) + (idx + 0.5) * W.RES
    lim, clr = R.LIMITS_OF[r], R.CLEARANCE
    path = tmp_path / "ragged_batch.bin"
    with open(path, "wb") as fh:
        fh.write(np.array([r, n, total, len(centres), *W.DIMS, lim["samples_per_seg"], clr["samples_per_seg"], 0], dtype=np.int32).tobytes())
        fh.write(np.array([*W.ORIGIN, W.RES, W.MAX_DIST, lim["v_max"], lim["a_max"], lim["weight_v"], lim["weight_a"], clr["d_safe"], clr["weight"],
                           R.PARAMS["max_move"]], dtype=np.float64).tobytes())
        fh.write(so.tobytes())
        for key in ("waypoints", "times", "bc"):
            fh.write(np.ascontiguousarray(b[key], dtype=np.float64).tobytes())
        fh.write(np.ascontiguousarray(centres, dtype=np.float64).tobytes())
    rocm = "/opt/rocm"
    exe = os.path.join(ROOT, "tests", "cpp", "test_spacetime_lbfgs_facade")
    pkg = os.path.join(ROOT, "uav_motion_planning_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-I", os.path.join(rocm, "include"), f"-I{pkg}/cpp",
                           os.path.join(ROOT, "tests", "cpp", "test_spacetime_lbfgs_facade.cpp"), f"-L{pkg}", "-luavqp", f"-Wl,-rpath,{pkg}",
                           f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib", "-o", exe])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "optimizeTrajectoryLbfgs: 14 trajectories" in out.stdout
