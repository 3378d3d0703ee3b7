// TrajOptimizer::setMovingObstacles, getMovingPenalty and optimizeTrajectoryMoving (cpp/traj_optimizer.h) with a uavqp::EsdfMap
// (cpp/esdf_map.h), in the style of test_attitude_opt_facade.cpp, on the RAGGED BATCH of the GPU tests: tests/test_gpu_moving_opt.py writes
// the batch (order, offsets, waypoints, durations, boundary derivatives), the centres of the scene's occupied voxels, the limits, the
// clearance, the attitude and the moving-obstacle parameters and the obstacle tracks into the file named by argv[1].  The facade
// reproduces uavqp_moving_penalty_host and uavqp_moving_optimize_host, called directly, byte for byte.  Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../uav_motion_planning_amd/cpp/esdf_map.h"
#include "../../uav_motion_planning_amd/cpp/traj_optimizer.h"

template <class T>
static bool take(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  uavqp_moving_params mp;
  uavqp_default_moving_params(&mp);
  if (mp.struct_size != (int32_t)sizeof(uavqp_moving_params) || mp.samples_per_seg != 8 || mp.d_safe != 1.0 || mp.downwash != 1.0 ||
      mp.weight != 1e3) return 1;
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  // header: r, n_traj, total segments, occupied voxels, dims[3], samples per segment of the limits, of the clearance, of the attitude and
  // of the moving penalty, n_obs, total obstacle segments, n_sets
  std::vector<int32_t> head, so, oso, set_off, traj_set;
  // origin[3], resolution, max_dist, v_max, a_max, weight_v, weight_a, d_safe, weight, max_move, gravity, f_min, f_max, tilt_max, rate_max,
  // weight_thrust, weight_tilt, weight_rate, moving d_safe, downwash, weight
  std::vector<double> num, wp, T, bc, occ, oT, oc, ostart, orad, tstart;
  if (!take(f, head, 14) || !take(f, num, 23)) return 2;
  const int r = head[0], n = head[1], total = head[2], n_occ = head[3], n_obs = head[11], ototal = head[12], n_sets = head[13];
  if ((r != 3 && r != 4) || n < 1 || total < n || n_occ < 1 || n_obs < 1 || ototal < n_obs || n_sets < 1) return 2;
  if (!take(f, so, (size_t)n + 1) || !take(f, wp, 3 * ((size_t)total + n)) || !take(f, T, (size_t)total) ||
      !take(f, bc, (size_t)n * 2 * (r - 1) * 3) || !take(f, occ, 3 * (size_t)n_occ)) return 2;
  if (!take(f, oso, (size_t)n_obs + 1) || !take(f, set_off, (size_t)n_sets + 1) || !take(f, traj_set, (size_t)n) || !take(f, oT, (size_t)ototal) ||
      !take(f, oc, (size_t)3 * 2 * r * ototal) || !take(f, ostart, (size_t)n_obs) || !take(f, orad, (size_t)n_obs) || !take(f, tstart, (size_t)n))
    return 2;
  std::fclose(f);
  if (so[0] != 0 || so[n] != total || oso[n_obs] != ototal) return 2;

  uavqp_clearance_params cp;
  uavqp_default_clearance_params(&cp);
  uavqp_limit_params lp;
  uavqp_default_limit_params(&lp);
  uavqp_attitude_params ap;
  uavqp_default_attitude_params(&ap);
  uavqp_spacetime_lbfgs_params pp;
  uavqp_default_spacetime_lbfgs_params(&pp);
  lp.samples_per_seg = head[7]; lp.v_max = num[5]; lp.a_max = num[6]; lp.weight_v = num[7]; lp.weight_a = num[8];
  cp.samples_per_seg = head[8]; cp.d_safe = num[9]; cp.weight = num[10];
  pp.max_move = num[11];
  ap.samples_per_seg = head[9]; ap.gravity = num[12]; ap.f_min = num[13]; ap.f_max = num[14]; ap.tilt_max = num[15]; ap.rate_max = num[16];
  ap.weight_thrust = num[17]; ap.weight_tilt = num[18]; ap.weight_rate = num[19];
  mp.samples_per_seg = head[10]; mp.d_safe = num[20]; mp.downwash = num[21]; mp.weight = num[22];
  uavqp_moving_obstacles mo;
  std::memset(&mo, 0, sizeof(mo));
  mo.struct_size = (int32_t)sizeof(mo);
  mo.n_obs = n_obs; mo.uniform_segments = 0; mo.n_sets = n_sets;
  mo.seg_offsets = oso.data(); mo.times = oT.data(); mo.coeff = oc.data(); mo.start = ostart.data(); mo.radius = orad.data();
  mo.set_offsets = set_off.data(); mo.traj_set = traj_set.data(); mo.traj_start = tstart.data();

  std::vector<int32_t> off(n + 1);   // waypoint-row offsets: one more knot than segments per trajectory
  for (int b = 0; b <= n; ++b) off[b] = so[b] + b;
  traj_optimization::TrajOptimizer opt(r);
  opt.setWaypoints(wp.data(), off.data(), n);
  opt.setTimeAllocation(T.data());
  opt.setBoundary(bc.data());
  if (!opt.getMovingPenalty(mp).empty()) return 3;   // no obstacles, nothing solved yet
  uavqp_moving_obstacles wrong = mo;
  wrong.struct_size = 8;
  if (opt.setMovingObstacles(&wrong)) return 3;
  wrong = mo;
  wrong.times = nullptr;
  if (opt.setMovingObstacles(&wrong)) return 3;
  if (!opt.setMovingObstacles(&mo)) return 3;
  if (!opt.getMovingPenalty(mp).empty()) return 3;   // nothing solved yet
  if (!opt.solve()) return 3;

  const int32_t dims[3] = {head[4], head[5], head[6]};
  uavqp::EsdfMap map(opt.context(), dims, num.data(), num[3], num[4]);
  if (!map.valid()) return 4;
  for (int k = 0; k < n_occ; ++k) map.setOccupied(&occ[3 * (size_t)k]);
  if (!map.updateESDF3d()) return 6;

  // the penalty of the start against the C ABI
  const std::vector<double> phi0 = opt.getMovingPenalty(mp);
  std::vector<double> phi1(n), gap1(n);
  std::vector<int32_t> near1(n);
  if (phi0.size() != (size_t)n) return 7;
  if (uavqp_moving_penalty_host(opt.context(), r, n, 0, so.data(), T.data(), opt.getPolyCoeff(), opt.status().data(), &mo, &mp, phi1.data(), nullptr,
                                nullptr, nullptr, gap1.data(), near1.data()) != UAVQP_OK) return 8;
  if (std::memcmp(phi0.data(), phi1.data(), sizeof(double) * n) != 0) return 9;
  if (std::memcmp(opt.minGap().data(), gap1.data(), sizeof(double) * n) != 0) return 10;
  if (std::memcmp(opt.nearestObstacle().data(), near1.data(), sizeof(int32_t) * n) != 0) return 10;
  int inside = 0;
  for (int b = 0; b < n; ++b) inside += phi0[b] > 0.0 && near1[b] >= set_off[traj_set[b]] && near1[b] < set_off[traj_set[b] + 1];
  if (inside != n) return 11;

  // the optimiser against the C ABI
  if (!opt.optimizeTrajectoryMoving(map, lp, cp, &ap, mp, &pp)) return 12;
  std::vector<double> wp2(wp), T2(T), coef2((size_t)3 * 2 * r * total, 0.0), obj2(2 * (size_t)n), pk2(2 * (size_t)n), md2(n), apk2(4 * (size_t)n),
      gap2(n);
  std::vector<int32_t> st2(n), acc2(n), out2(n), near2(n);
  if (uavqp_moving_optimize_host(opt.context(), r, n, 0, 0, so.data(), wp2.data(), T2.data(), bc.data(), map.handle(), &lp, &cp, &ap, &mo, &mp, &pp,
                                 coef2.data(), st2.data(), obj2.data(), acc2.data(), pk2.data(), md2.data(), out2.data(), apk2.data(), gap2.data(),
                                 near2.data()) != UAVQP_OK) return 13;
  if (std::memcmp(opt.waypoints().data(), wp2.data(), sizeof(double) * wp2.size()) != 0) return 14;
  if (std::memcmp(opt.timeAllocation().data(), T2.data(), sizeof(double) * T2.size()) != 0) return 24;
  if (std::memcmp(opt.getPolyCoeff(), coef2.data(), sizeof(double) * coef2.size()) != 0) return 15;
  if (std::memcmp(opt.objective().data(), obj2.data(), sizeof(double) * obj2.size()) != 0) return 16;
  if (std::memcmp(opt.acceptedTrials().data(), acc2.data(), sizeof(int32_t) * n) != 0) return 17;
  if (std::memcmp(opt.minDist().data(), md2.data(), sizeof(double) * n) != 0 || std::memcmp(opt.outsideSamples().data(), out2.data(), sizeof(int32_t) * n) != 0) return 18;
  if (std::memcmp(opt.peak().data(), pk2.data(), sizeof(double) * pk2.size()) != 0) return 25;
  if (std::memcmp(opt.attitudePeak().data(), apk2.data(), sizeof(double) * apk2.size()) != 0) return 26;
  if (std::memcmp(opt.minGap().data(), gap2.data(), sizeof(double) * n) != 0) return 32;
  if (std::memcmp(opt.nearestObstacle().data(), near2.data(), sizeof(int32_t) * n) != 0) return 33;
  if (std::memcmp(opt.status().data(), st2.data(), sizeof(int32_t) * n) != 0) return 19;
  const std::vector<double>& obj = opt.objective();
  double ratio = 0.0;
  for (int b = 0; b < n; ++b) {
    if (!(obj[2 * b + 1] < obj[2 * b]) || opt.acceptedTrials()[b] < 1) return 20;
    ratio = std::fmax(ratio, obj[2 * b + 1] / obj[2 * b]);
  }
  // the start objective carries the start's moving penalty: the parent entry's is smaller by exactly that much, up to rounding
  traj_optimization::TrajOptimizer plain(r);
  plain.setWaypoints(wp.data(), off.data(), n);
  plain.setTimeAllocation(T.data());
  plain.setBoundary(bc.data());
  uavqp::EsdfMap map2(plain.context(), dims, num.data(), num[3], num[4]);
  if (!map2.valid()) return 4;
  for (int k = 0; k < n_occ; ++k) map2.setOccupied(&occ[3 * (size_t)k]);
  if (!map2.updateESDF3d()) return 6;
  if (!plain.optimizeTrajectoryAttitude(map2, lp, cp, ap, &pp)) return 27;
  for (int b = 0; b < n; ++b)
    if (std::fabs(plain.objective()[2 * b] + phi0[b] - obj[2 * b]) > 1e-12 * obj[2 * b]) return 28;
  std::printf("optimizeTrajectoryMoving: %d trajectories, %d with a track inside D_o at the start, largest f_result / f_start %.4f\n", n, inside,
              ratio);
  // invalid parameters are refused; without obstacles there is nothing to optimise against; corridor problems are out of scope
  uavqp_moving_params bad = mp;
  bad.downwash = 0.5;
  if (opt.optimizeTrajectoryMoving(map, lp, cp, &ap, bad, &pp)) return 29;
  if (!opt.getMovingPenalty(bad).empty()) return 31;
  if (plain.optimizeTrajectoryMoving(map2, lp, cp, &ap, mp, &pp)) return 34;
  std::vector<double> lo(wp.size(), 0.0), hi(wp.size(), 0.0);
  opt.setCorridor(lo.data(), hi.data());
  if (opt.optimizeTrajectoryMoving(map, lp, cp, &ap, mp, &pp)) return 30;
  return 0;
}
