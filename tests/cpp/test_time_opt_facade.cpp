// TrajOptimizer::optimizeTime / getCost through the drop-in header (cpp/traj_optimizer.h), in the style of test_qpsolve_mirror.cpp.
// One rest-to-rest segment has a closed form: J = C_r |D|^2 / T^(2r-1) (C_3 = 720), f = J + w T minimal at T* = ((2r-1) C_r |D|^2 / w)^(1/2r);
// a three-segment path with uneven spacing from the reference's T = 1.0 must lose objective and stay self-consistent.  Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../uav_motion_planning_amd/cpp/traj_optimizer.h"

int main() {
  const double w = 50.0;
  {
    traj_optimization::TrajOptimizer opt(3);
    const double xyz[6] = {0.0, 0.0, 0.0, 3.0, -4.0, 12.0};   // |D| = 13
    const int32_t off[2] = {0, 2};
    const double T[1] = {1.0};
    opt.setWaypoints(xyz, off, 1);
    opt.setTimeAllocation(T);
    if (!opt.solve()) return 1;
    std::vector<double> c0 = opt.getCost();
    if (c0.size() != 1 || std::fabs(c0[0] - 720.0 * 169.0) > 1e-9 * 720.0 * 169.0) { std::printf("getCost %.17g\n", c0.empty() ? -1.0 : c0[0]); return 2; }
    if (!opt.optimizeTime(w)) return 3;
    const double A = 720.0 * 169.0, T_star = std::pow(5.0 * A / w, 1.0 / 6.0), f_star = A / std::pow(T_star, 5) + w * T_star, f_start = A + w;
    const double f0 = opt.objective()[0], f1 = opt.objective()[1], T1 = opt.timeAllocation()[0];
    const double gap = (f1 - f_star) / (f_start - f_star);
    std::printf("optimizeTime one segment: T %.6f (T* %.6f), f %.6f -> %.6f (f* %.6f), gap %.3e, %d trials accepted\n", T1, T_star, f0, f1, f_star, gap,
                opt.acceptedTrials()[0]);
    if (std::fabs(f0 - f_start) > 1e-9 * f_start) return 4;
    if (!(f1 <= f0) || !(f1 >= f_star * (1.0 - 1e-9)) || !(gap <= 0.05)) return 5;
    std::vector<double> c1 = opt.getCost();   // the cost AT the optimised durations: objective minus the time term
    if (c1.size() != 1 || std::fabs(c1[0] + w * T1 - f1) > 1e-12 * f1) return 6;
  }
  {
    traj_optimization::TrajOptimizer opt(4);
    const double xyz[12] = {0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 2.5, 1.0, 0.0, 2.5, 5.0, 1.0};
    const int32_t off[2] = {0, 4};
    const double T[3] = {1.0, 1.0, 1.0};
    opt.setWaypoints(xyz, off, 1);
    opt.setTimeAllocation(T);
    if (!opt.optimizeTime(w)) return 7;
    const double f0 = opt.objective()[0], f1 = opt.objective()[1];
    std::printf("optimizeTime three segments: f %.6f -> %.6f, T = %.4f %.4f %.4f\n", f0, f1, opt.timeAllocation()[0], opt.timeAllocation()[1],
                opt.timeAllocation()[2]);
    if (!(f1 < 0.5 * f0)) return 8;
    // getPolyCoeff() is the solve at timeAllocation(): solving again changes nothing
    std::vector<double> c(opt.getPolyCoeff(), opt.getPolyCoeff() + 3 * 3 * 8);
    if (!opt.solve()) return 9;
    for (int i = 0; i < 72; ++i) if (opt.getPolyCoeff()[i] != c[i]) return 10;
    // out of scope: corridor problems
    double lo[12], hi[12];
    for (int i = 0; i < 12; ++i) { lo[i] = xyz[i] - 0.1; hi[i] = xyz[i] + 0.1; }
    opt.setCorridor(lo, hi);
    if (opt.optimizeTime(w)) return 11;
  }
  return 0;
}
