// TrajOptimizer::optimizeSwarm (cpp/traj_optimizer.h) with a uavqp::EsdfMap (cpp/esdf_map.h), in the style of test_spacetime_facade.cpp and
// test_swarm_facade.cpp.  A 24 x 20 x 12 map with a pillar from a cloud; five trajectories in two swarms (3 + 2) whose paths cross,
// staggered departures inside a window.  The facade reproduces uavqp_swarm_optimize_host, called directly, byte for byte; the objectives
// are printed with 17 digits so that tests/test_gpu_swarm_opt_facade.py can compare them with the Python facade's on the same batch.
// Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../uav_motion_planning_amd/cpp/esdf_map.h"
#include "../../uav_motion_planning_amd/cpp/traj_optimizer.h"

int main() {
  uavqp_swarm_opt_params pp;
  uavqp_default_swarm_opt_params(&pp);
  uavqp_spacetime_params sp0;
  uavqp_default_spacetime_params(&sp0);
  if (pp.struct_size != (int32_t)sizeof(uavqp_swarm_opt_params) || pp.max_iters != sp0.max_iters || pp.smooth_weight != 1.0 ||
      pp.time_weight != 50.0 || pp.t_min != 1e-2 || pp.t_max != 1e2 || pp.max_move != 2.0 || pp.initial_step_move != 0.1 ||
      pp.initial_step_log != 0.1 || pp.armijo_c != 1e-4 || pp.shrink != 0.5 || pp.grow != 2.0 || pp.start_window != 0.0 ||
      pp.initial_step_start != 0.1) return 1;
  uavqp_clearance_params cp;
  uavqp_default_clearance_params(&cp);
  uavqp_limit_params lp;
  uavqp_default_limit_params(&lp);
  lp.v_max = 1.5;
  lp.a_max = 2.0;
  uavqp_swarm_params sw;
  uavqp_default_swarm_params(&sw);
  sw.n_samples = 60;
  sw.clock_start = -0.3;
  sw.d_safe = 0.9;

  // 14 knots: 3 + 2 + 1 | 2 + 1 segments (the batch of test_swarm_facade.cpp, flown more slowly)
  const double xyz[42] = {-1.5, 0.0, 1.0, -0.5, 0.1, 1.1, 0.5, -0.1, 1.0, 1.5, 0.0, 1.0,
                          0.0, -1.5, 1.2, 0.1, 0.0, 1.1, 0.0, 1.5, 1.0,
                          1.2, 1.2, 0.9, -1.2, -1.2, 1.1,
                          -2.5, -1.0, 1.0, -1.5, -0.7, 1.0, -0.5, -1.0, 1.0,
                          -1.5, 0.2, 1.1, -1.5, -2.2, 0.9};
  const int32_t off[6] = {0, 4, 7, 9, 12, 14};
  const int32_t so[6] = {0, 3, 5, 6, 8, 9};
  const double T[9] = {1.1, 1.0, 1.1, 1.6, 1.5, 3.0, 1.4, 1.5, 2.6};
  const int32_t groups[3] = {0, 3, 5};
  const double start[5] = {0.0, 0.15, -0.2, 0.3, 0.0};
  traj_optimization::TrajOptimizer opt(3);
  opt.setWaypoints(xyz, off, 5);
  opt.setTimeAllocation(T);
  opt.setSwarm(groups, 2, start);
  if (!opt.solve()) return 3;

  const int32_t dims[3] = {24, 20, 12};
  const double origin[3] = {-3.0, -2.5, 0.0};
  uavqp::EsdfMap map(opt.context(), dims, origin, 0.25);
  if (!map.valid()) return 4;
  std::vector<double> cloud;
  for (int k = 0; k < 14; ++k) { cloud.push_back(1.03); cloud.push_back(0.61); cloud.push_back(0.07 + 0.21 * k); }
  if (!map.setCloud(cloud.data(), 14, 0.25)) return 5;
  if (!map.updateESDF3d()) return 6;

  pp.max_iters = 16;
  pp.max_move = 1.0;
  pp.time_weight = 30.0;
  pp.start_window = 0.25;
  if (!opt.optimizeSwarm(map, lp, cp, sw, &pp)) return 12;
  std::vector<double> wp2(xyz, xyz + 42), T2(T, T + 9), s2(start, start + 5), coef2(3 * 6 * 9, 0.0), obj2(4), pk2(10), md2(5), ms2(5);
  std::vector<int32_t> st2(5), acc2(2), out2(5);
  const std::vector<double> bc(5 * 2 * 2 * 3, 0.0);
  if (uavqp_swarm_optimize_host(opt.context(), 3, 5, 0, 0, so, wp2.data(), T2.data(), bc.data(), 2, groups, s2.data(), map.handle(), &lp, &cp, &sw,
                                &pp, coef2.data(), st2.data(), obj2.data(), acc2.data(), pk2.data(), md2.data(), out2.data(),
                                ms2.data()) != UAVQP_OK) return 13;
  if (std::memcmp(opt.waypoints().data(), wp2.data(), sizeof(double) * 42) != 0) return 14;
  if (std::memcmp(opt.timeAllocation().data(), T2.data(), sizeof(double) * 9) != 0) return 15;
  if (opt.swarmStart().size() != 5 || std::memcmp(opt.swarmStart().data(), s2.data(), sizeof(double) * 5) != 0) return 16;
  if (std::memcmp(opt.getPolyCoeff(), coef2.data(), sizeof(double) * coef2.size()) != 0) return 17;
  if (opt.objective().size() != 4 || std::memcmp(opt.objective().data(), obj2.data(), sizeof(double) * 4) != 0) return 18;
  if (opt.acceptedTrials().size() != 2 || std::memcmp(opt.acceptedTrials().data(), acc2.data(), sizeof(int32_t) * 2) != 0) return 19;
  if (std::memcmp(opt.minDist().data(), md2.data(), sizeof(double) * 5) != 0 || std::memcmp(opt.outsideSamples().data(), out2.data(), sizeof(int32_t) * 5) != 0) return 20;
  if (std::memcmp(opt.peak().data(), pk2.data(), sizeof(double) * 10) != 0) return 21;
  if (opt.minSep().size() != 5 || std::memcmp(opt.minSep().data(), ms2.data(), sizeof(double) * 5) != 0) return 22;
  if (std::memcmp(opt.status().data(), st2.data(), sizeof(int32_t) * 5) != 0) return 23;
  const std::vector<double>& obj = opt.objective();
  for (int g = 0; g < 2; ++g)
    if (!(obj[2 * g + 1] < obj[2 * g]) || opt.acceptedTrials()[g] < 1) return 24;
  // the departures moved, inside the window; the end knots come back byte for byte
  bool moved = false;
  for (int b = 0; b < 5; ++b) {
    if (!(opt.swarmStart()[b] >= start[b] - 0.25 && opt.swarmStart()[b] <= start[b] + 0.25)) return 25;
    moved = moved || opt.swarmStart()[b] != start[b];
  }
  if (!moved) return 26;
  const int ends[10] = {0, 3, 4, 6, 7, 8, 9, 11, 12, 13};
  for (int k : ends)
    if (std::memcmp(&opt.waypoints()[3 * k], &xyz[3 * k], 24) != 0) return 27;
  std::printf("optimizeSwarm OK %.17g %.17g %.17g %.17g accepted %d %d\n", obj[0], obj[1], obj[2], obj[3], opt.acceptedTrials()[0],
              opt.acceptedTrials()[1]);
  // invalid parameters and offsets are refused
  uavqp_swarm_opt_params bad = pp;
  bad.start_window = -1.0;
  if (opt.optimizeSwarm(map, lp, cp, sw, &bad)) return 28;
  const int32_t wrong[3] = {0, 4, 4};
  opt.setSwarm(wrong, 2, start);
  if (opt.optimizeSwarm(map, lp, cp, sw, &pp)) return 29;
  opt.setSwarm(groups, 2, start);
  const double lo[42] = {0}, hi[42] = {0};
  opt.setCorridor(lo, hi);
  if (opt.optimizeSwarm(map, lp, cp, sw, &pp)) return 30;           // corridor problems are out of scope
  return 0;
}
