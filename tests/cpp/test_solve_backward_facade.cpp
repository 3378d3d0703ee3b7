// TrajOptimizer::backward through the drop-in header (cpp/traj_optimizer.h), in the style of test_time_opt_facade.cpp.
// One rest-to-rest min-jerk segment has a closed form: p(t) = p0 + D (10 s^3 - 15 s^4 + 6 s^5), s = t / T, i.e. c3 = 10 D / T^3,
// c4 = -15 D / T^4, c5 = 6 D / T^5, c0 = p0 -- the gradients of g . c follow by hand; a three-segment min-snap path is checked against
// central differences through solve() itself.  Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../uav_motion_planning_amd/cpp/traj_optimizer.h"

static bool close(double a, double b, double tol, double scale) { return std::fabs(a - b) <= tol * scale; }

int main() {
  {
    traj_optimization::TrajOptimizer opt(3);
    const double xyz[6] = {1.0, 2.0, 3.0, 4.0, -2.0, 15.0};
    const int32_t off[2] = {0, 2};
    const double T[1] = {1.7};
    opt.setWaypoints(xyz, off, 1);
    opt.setTimeAllocation(T);
    std::vector<double> g(18), gT, gW, gB;
    for (int i = 0; i < 18; ++i) g[i] = std::sin(1.0 + 0.7 * i);
    if (opt.backward(g, gT, gW, gB)) return 1;   // before solve(): refused
    if (!opt.solve()) return 2;
    if (!opt.backward(g, gT, gW, gB)) return 3;
    if (gT.size() != 1 || gW.size() != 6 || gB.size() != 12) return 4;
    const double t = T[0];
    double wantT = 0.0, scaleT = 0.0;
    for (int ax = 0; ax < 3; ++ax) {
      const double D = xyz[3 + ax] - xyz[ax], *ga = &g[6 * ax];
      const double term = ga[3] * (-30.0 * D / std::pow(t, 4)) + ga[4] * (60.0 * D / std::pow(t, 5)) + ga[5] * (-30.0 * D / std::pow(t, 6));
      wantT += term;
      scaleT += std::fabs(term);
      const double e = ga[3] * 10.0 / std::pow(t, 3) - ga[4] * 15.0 / std::pow(t, 4) + ga[5] * 6.0 / std::pow(t, 5);
      if (!close(gW[3 + ax], e, 1e-12, std::fabs(e) + 1.0) || !close(gW[ax], ga[0] - e, 1e-12, std::fabs(e) + 1.0)) return 5;
    }
    std::printf("backward one segment: grad T %.12g (closed form %.12g)\n", gT[0], wantT);
    if (!close(gT[0], wantT, 1e-12, scaleT)) return 6;
  }
  {
    traj_optimization::TrajOptimizer opt(4);
    const double xyz[12] = {0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 2.5, 1.0, 0.0, 2.5, 5.0, 1.0};
    const int32_t off[2] = {0, 4};
    const double T[3] = {0.8, 1.3, 1.9};
    std::vector<double> bc(18);
    for (int i = 0; i < 18; ++i) bc[i] = 0.3 * std::cos(2.0 + i);
    opt.setWaypoints(xyz, off, 1);
    opt.setBoundary(bc.data());
    opt.setTimeAllocation(T);
    if (!opt.solve()) return 7;
    std::vector<double> g(72), gT, gW, gB;
    for (int i = 0; i < 72; ++i) g[i] = std::sin(0.3 + 1.1 * i);
    if (!opt.backward(g, gT, gW, gB)) return 8;
    auto phi = [&](const double* xyz_, const double* T_, const double* bc_) -> double {
      traj_optimization::TrajOptimizer o(4);
      o.setWaypoints(xyz_, off, 1);
      o.setBoundary(bc_);
      o.setTimeAllocation(T_);
      if (!o.solve()) return NAN;
      double s = 0.0;
      for (int i = 0; i < 72; ++i) s += g[i] * o.getPolyCoeff()[i];
      return s;
    };
    double worst = 0.0, scale = 0.0;
    for (int i = 0; i < 3; ++i) scale = std::fmax(scale, std::fabs(gT[i]));
    for (int i = 0; i < 3; ++i) {
      double Tp[3] = {T[0], T[1], T[2]}, Tm[3] = {T[0], T[1], T[2]};
      const double h = 1e-5 * T[i];
      Tp[i] += h;
      Tm[i] -= h;
      const double fd = (phi(xyz, Tp, bc.data()) - phi(xyz, Tm, bc.data())) / (2.0 * h);
      worst = std::fmax(worst, std::fabs(fd - gT[i]) / scale);
    }
    // c* is linear in the waypoints and the boundary derivatives: one difference each, any step
    double sw = 0.0, ww = 0.0;
    for (int k = 0; k < 12; ++k) sw = std::fmax(sw, std::fabs(gW[k]));
    for (int k = 0; k < 12; ++k) {
      double xp[12], xm[12];
      for (int j = 0; j < 12; ++j) xp[j] = xm[j] = xyz[j];
      xp[k] += 0.5;
      xm[k] -= 0.5;
      ww = std::fmax(ww, std::fabs(phi(xp, T, bc.data()) - phi(xm, T, bc.data()) - gW[k]) / sw);
    }
    double sb = 0.0, wb = 0.0;
    for (int k = 0; k < 18; ++k) sb = std::fmax(sb, std::fabs(gB[k]));
    for (int k = 0; k < 18; ++k) {
      std::vector<double> bp(bc), bm(bc);
      bp[k] += 0.5;
      bm[k] -= 0.5;
      wb = std::fmax(wb, std::fabs(phi(xyz, T, bp.data()) - phi(xyz, T, bm.data()) - gB[k]) / sb);
    }
    std::printf("backward three segments: worst |fd - grad| / max|grad|: times %.3e, waypoints %.3e, bc %.3e\n", worst, ww, wb);
    // central differences in double through the device solve: truncation ~1e-10, rounding ~1e-16 * cancellation / 1e-5
    if (!(worst <= 1e-6) || !(ww <= 1e-8) || !(wb <= 1e-8)) return 9;
    // out of scope: corridor problems
    double lo[12], hi[12];
    for (int i = 0; i < 12; ++i) { lo[i] = xyz[i] - 0.1; hi[i] = xyz[i] + 0.1; }
    opt.setCorridor(lo, hi);
    if (opt.backward(g, gT, gW, gB)) return 10;
  }
  return 0;
}
