"""-m gpu: the facades of the swarm optimiser -- Python TrajOptimizer.optimizeSwarm and the C++ TrajOptimizer::optimizeSwarm of
cpp/traj_optimizer.h with the uavqp::EsdfMap of cpp/esdf_map.h (tests/cpp/test_swarm_opt_facade.cpp, built and run the way
tests/test_gpu_spacetime_facade.py does): both reproduce the C-ABI outputs byte for byte on a batch of two swarms."""
import os
import subprocess

import numpy as np
import pytest

import uav_motion_planning_amd as U
from uav_motion_planning_amd.esdf import EsdfMap

import spacetime_reference as R
import swarm_opt_reference as O
import waypoint_opt_reference as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_facade_optimize_swarm():
    b = O.batch(3, ((3, 1, 4), (2, 5)), 5)
    so, go = b["seg_offsets"], b["group_offsets"]
    lim, clr, sw = dict(O.LIMITS), dict(d_safe=0.6), dict(O.SWARM)
    par = dict(max_move=1.0, max_iters=12, time_weight=30.0, start_window=0.2)
    opt = U.TrajOptimizer(order=3)
    opt.setWaypoints(b["waypoints"], wp_offsets=so + np.arange(so.size))
    opt.setTimeAllocation(b["times"])
    opt.setBoundary(b["bc"])
    opt.setSwarm(group_offsets=go, start_times=b["start"])
    ctx = opt.context()
    sc = R.scene()
    with EsdfMap(ctx, W.DIMS, W.ORIGIN, W.RES, W.MAX_DIST) as m:
        m.set_occupancy(sc["occ"])
        m.update()
        assert opt.solve() is True
        phi0 = opt.getSwarmPenalty(**sw)
        assert np.all(phi0 > 0.0)
        want = ctx.swarm_optimize_host(3, so, b["waypoints"], b["times"], b["bc"], m, group_offsets=go, start=b["start"], limits=lim,
                                       clearance=clr, swarm=sw, **par)
        assert opt.optimizeSwarm(m, limits=lim, clearance=clr, swarm=sw, **par) is True
        got = (opt.getWaypoints(), opt.getTimeAllocation(), opt.getSwarmStart(), opt.getPolyCoeff(), opt.status, opt.objective, opt.iterations,
               opt.peak, opt.min_dist, opt.outside, opt.min_sep)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        assert opt.objective.shape == (2, 2) and opt.iterations.shape == (2,)
        assert np.all(opt.objective[:, 1] < opt.objective[:, 0]) and np.all(opt.iterations > 0)
        assert np.any(opt.getSwarmStart() != b["start"]) and np.all(np.abs(opt.getSwarmStart() - b["start"]) <= 0.2 + 1e-12)
        # the new departures are stored: the swarm penalty of the facade is taken at them
        assert opt.solve() is True
        phi1 = opt.getSwarmPenalty(**sw)
        assert phi1.tobytes() == ctx.swarm_penalty_host(3, so, opt.getTimeAllocation(), opt.getPolyCoeff(), group_offsets=go, start=opt.getSwarmStart(),
                                                        status=opt.status, **sw)[0].tobytes()
        assert np.all(phi1 < phi0)
        # without departures and with the window closed the facade passes none
        opt.setSwarm(group_offsets=go)
        assert opt.optimizeSwarm(m, limits=lim, clearance=clr, swarm=sw, max_iters=2) is True and opt.getSwarmStart() is None
        with pytest.raises(ValueError):
            opt.optimizeSwarm(m, no_such_field=1.0)
        opt.setCorridor(b["waypoints"] - 0.1, b["waypoints"] + 0.1)
        with pytest.raises(ValueError):
            opt.optimizeSwarm(m)


def test_cpp_facade_optimize_swarm():
    """TrajOptimizer::optimizeSwarm agrees with the C ABI."""
    rocm = "/opt/rocm"
    exe = os.path.join(ROOT, "tests", "cpp", "test_swarm_opt_facade")
    pkg = os.path.join(ROOT, "uav_motion_planning_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-I", os.path.join(rocm, "include"), f"-I{pkg}/cpp",
                           os.path.join(ROOT, "tests", "cpp", "test_swarm_opt_facade.cpp"), f"-L{pkg}", "-luavqp", f"-Wl,-rpath,{pkg}",
                           f"-L{rocm}/lib", "-lamdhip64", f"-Wl,-rpath,{rocm}/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "optimizeSwarm OK" in out.stdout
