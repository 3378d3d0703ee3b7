"""-m gpu: the facades of the joint optimiser -- Python TrajOptimizer.optimizeTrajectory / getFlightPenalty and the C++ TrajOptimizer of
cpp/traj_optimizer.h with the uavqp::EsdfMap of cpp/esdf_map.h (tests/cpp/test_spacetime_facade.cpp, built and run the way
tests/test_gpu_waypoint_opt_facade.py does): both reproduce the C-ABI outputs byte for byte on a batch of four trajectories."""
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


def test_python_facade_optimize_trajectory():
    b = W.cases(3, Ms=[3, 5, 1, 4])
    so = b["seg_offsets"]
    lim, clr, par = dict(R.LIMITS_OF[3]), dict(d_safe=0.6), dict(max_move=1.0, max_iters=16, time_weight=30.0)
    opt = U.TrajOptimizer(order=3)
    opt.setWaypoints(b["waypoints"], wp_offsets=so + np.arange(so.size))
    opt.setTimeAllocation(b["times"])
    opt.setBoundary(b["bc"])
    ctx = opt.context()
    sc = R.scene()
    with EsdfMap(ctx, W.DIMS, W.ORIGIN, W.RES, W.MAX_DIST) as m:
        m.set_occupancy(sc["occ"])
        m.update()
        with pytest.raises(U.UavqpError):
            opt.getFlightPenalty(m)                                     # before a solve
        assert opt.solve() is True
        phi0 = opt.getFlightPenalty(m, limits=lim, clearance=clr)
        assert phi0.tobytes() == ctx.flight_penalty_host(3, so, b["times"], opt.getPolyCoeff(), m, status=opt.status, limits=lim, clearance=clr)[0].tobytes()
        assert np.all(phi0 > 0.0)
        want = ctx.spacetime_optimize_host(3, so, b["waypoints"], b["times"], b["bc"], m, limits=lim, clearance=clr, **par)
        assert opt.optimizeTrajectory(m, limits=lim, clearance=clr, **par) is True
        got = (opt.getWaypoints(), opt.getTimeAllocation(), opt.getPolyCoeff(), opt.status, opt.objective, opt.iterations, opt.peak, opt.min_dist,
               opt.outside)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        assert np.all(opt.objective[:, 1] < opt.objective[:, 0]) and np.all(opt.outside == 0) and np.all(opt.iterations > 0)
        assert np.any(opt.getWaypoints() != b["waypoints"]) and np.all(opt.getTimeAllocation() != b["times"])
        # getPolyCoeff stays valid: it is the solve at the stored waypoints and durations
        coef = opt.getPolyCoeff()
        assert opt.solve() is True and np.array_equal(opt.getPolyCoeff(), coef)
        assert np.all(opt.getFlightPenalty(m, limits=lim, clearance=clr) < phi0)
        with pytest.raises(ValueError):
            opt.optimizeTrajectory(m, no_such_field=1.0)
        opt.setCorridor(b["waypoints"] - 0.1, b["waypoints"] + 0.1)
        with pytest.raises(ValueError):
            opt.optimizeTrajectory(m)


def test_cpp_facade_optimize_trajectory():
    """TrajOptimizer::optimizeTrajectory / getFlightPenalty agree with the C ABI."""
    rocm = "/opt/rocm"
    exe = os.path.join(ROOT, "tests", "cpp", "test_spacetime_facade")
    pkg = os.path.join(ROOT, "uav_motion_planning_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-I", os.path.join(rocm, "include"), f"-I{pkg}/cpp",
                           os.path.join(ROOT, "tests", "cpp", "test_spacetime_facade.cpp"), f"-L{pkg}", "-luavqp", f"-Wl,-rpath,{pkg}",
                           f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "optimizeTrajectory" in out.stdout
