// kernel_instances.h -- which kernel instantiations live in which translation unit (round 6).
//
// libuavqp.so used to be ONE translation unit (uavqp.hip, 80-90 s of hipcc for every one-line change).  The register-heavy solver families
// are now compiled on their own (k_*.hip, `make -j`): each family file defines UAVQP_KERNEL_TU, includes its header and this file, and
// expands ITS list with UAVQP_INST = explicit instantiation definition; the host translation unit (uavqp.hip) expands EVERY list with
// UAVQP_INST = explicit instantiation declaration (`extern template`), so its launch sites -- unchanged hipLaunchKernelGGL calls -- bind
// to the family's kernels at link time and nothing is compiled twice.  An instantiation that is launched but missing from these lists is
// simply instantiated by the host translation unit, as before (slower to build, same library).
// Plain (non-template) kernels are emitted by the host translation unit only (#ifndef UAVQP_KERNEL_TU around their definitions).
#pragma once

#ifdef UAVQP_KERNEL_TU
#define UAVQP_INST template
#else
#define UAVQP_INST extern template
#endif

// ---- qp_twisted.h: solve_twisted_kernel<R, M, TILE, LPT, ONE>, the (R, M) pairs of find_twisted() x the four tile shapes
// (UAVQP_TWISTED_SIG: the one flat parameter list of the family, qp_twisted.h)
#define UAVQP_TWISTED_SHAPES(R_, M_)                                                          \
    UAVQP_INST __global__ void uavqp::solve_twisted_kernel<R_, M_, 4, 16>(UAVQP_TWISTED_SIG);     \
    UAVQP_INST __global__ void uavqp::solve_twisted_kernel<R_, M_, 8, 8>(UAVQP_TWISTED_SIG);      \
    UAVQP_INST __global__ void uavqp::solve_twisted_kernel<R_, M_, 16, 2>(UAVQP_TWISTED_SIG);     \
    UAVQP_INST __global__ void uavqp::solve_twisted_kernel<R_, M_, 32, 2>(UAVQP_TWISTED_SIG);
// (two translation units, k_twisted3.hip / k_twisted4.hip: 80 instantiations are the longest compile of the library)
#define UAVQP_TWISTED_PAIRS4(X) X(4, 2) X(4, 3) X(4, 4) X(4, 5) X(4, 6) X(4, 7) X(4, 8) X(4, 9) X(4, 10) X(4, 12)
#define UAVQP_TWISTED_PAIRS3(X) X(3, 2) X(3, 3) X(3, 4) X(3, 5) X(3, 6) X(3, 7) X(3, 8) X(3, 10) X(3, 12) X(3, 16)
#define UAVQP_INSTANCES_TWISTED3 UAVQP_TWISTED_PAIRS3(UAVQP_TWISTED_SHAPES)
#define UAVQP_INSTANCES_TWISTED4 UAVQP_TWISTED_PAIRS4(UAVQP_TWISTED_SHAPES)
// the latency shapes once more for launches of exactly one whole tile per wave (ONE = true; k_twisted3_one.hip / k_twisted4_one.hip)
#define UAVQP_TWISTED_SHAPES_ONE(R_, M_)                                                            \
    UAVQP_INST __global__ void uavqp::solve_twisted_kernel<R_, M_, 4, 16, true>(UAVQP_TWISTED_SIG); \
    UAVQP_INST __global__ void uavqp::solve_twisted_kernel<R_, M_, 8, 8, true>(UAVQP_TWISTED_SIG);
#define UAVQP_INSTANCES_TWISTED3_ONE UAVQP_TWISTED_PAIRS3(UAVQP_TWISTED_SHAPES_ONE)
#define UAVQP_INSTANCES_TWISTED4_ONE UAVQP_TWISTED_PAIRS4(UAVQP_TWISTED_SHAPES_ONE)
// and the group kernel, several one-tile-per-wave solves in one launch (k_twisted3_group.hip / k_twisted4_group.hip), for those of the
// latency shapes whose wave fits THREE to a SIMD: at most 168 VGPRs, no scratch (the group kernel has the register count of the
// one-tile-per-wave kernel of its shape: both are qp_twisted_body.h; tests/test_capture_fuse.py reads the counts from a cross-compile).
// The others -- 16 lanes: (4, 7) 182, (4, 9) 210, (4, 10) 182, (4, 12) 216;  8 lanes: (4, 5) 190, (4, 7) 228, (4, 8) 200, (4, 9) 264, (4, 10) 240,
// (4, 12) 266, (3, 12) 184, (3, 16) 234 -- have no group kernel and are replayed one launch per solve.
#define UAVQP_GROUP_PAIRS4_T4(X) X(4, 2) X(4, 3) X(4, 4) X(4, 5) X(4, 6) X(4, 8)
#define UAVQP_GROUP_PAIRS4_T8(X) X(4, 2) X(4, 3) X(4, 4) X(4, 6)
#define UAVQP_GROUP_PAIRS3_T4(X) UAVQP_TWISTED_PAIRS3(X)
#define UAVQP_GROUP_PAIRS3_T8(X) X(3, 2) X(3, 3) X(3, 4) X(3, 5) X(3, 6) X(3, 7) X(3, 8) X(3, 10)
#define UAVQP_TWISTED_GROUP_T4(R_, M_) UAVQP_INST __global__ void uavqp::solve_twisted_group_kernel<R_, M_, 4, 16>(UAVQP_TWISTED_GROUP_SIG);
#define UAVQP_TWISTED_GROUP_T8(R_, M_) UAVQP_INST __global__ void uavqp::solve_twisted_group_kernel<R_, M_, 8, 8>(UAVQP_TWISTED_GROUP_SIG);
#define UAVQP_INSTANCES_TWISTED3_GROUP UAVQP_GROUP_PAIRS3_T4(UAVQP_TWISTED_GROUP_T4) UAVQP_GROUP_PAIRS3_T8(UAVQP_TWISTED_GROUP_T8)
#define UAVQP_INSTANCES_TWISTED4_GROUP UAVQP_GROUP_PAIRS4_T4(UAVQP_TWISTED_GROUP_T4) UAVQP_GROUP_PAIRS4_T8(UAVQP_TWISTED_GROUP_T8)
// and the group of tile-4 solves with eight trajectories per wave (solve_twisted_group8_kernel; k_twisted3_group8.hip / k_twisted4_group8.hip):
// every shape of the tile-4 group lists -- all of them compile without scratch and fit THREE waves to a SIMD (at most 168 VGPRs, at
// most a twelfth of a CU's LDS; tests/test_twisted_group8_three_waves.py reads the counts from a cross-compile, docs/measurement_log.md
// tables them).
#define UAVQP_GROUP8_PAIRS4(X) UAVQP_GROUP_PAIRS4_T4(X)
#define UAVQP_GROUP8_PAIRS3(X) UAVQP_GROUP_PAIRS3_T4(X)
#define UAVQP_TWISTED_GROUP8(R_, M_) UAVQP_INST __global__ void uavqp::solve_twisted_group8_kernel<R_, M_>(UAVQP_TWISTED_GROUP8_SIG);
#define UAVQP_INSTANCES_TWISTED3_GROUP8 UAVQP_GROUP8_PAIRS3(UAVQP_TWISTED_GROUP8)
#define UAVQP_INSTANCES_TWISTED4_GROUP8 UAVQP_GROUP8_PAIRS4(UAVQP_TWISTED_GROUP8)
static inline bool uavqp_twisted_group8_exists(int r, int M) {
#define UAVQP_GROUP_HAS(R_, M_) if (r == R_ && M == M_) return true;
    UAVQP_GROUP8_PAIRS4(UAVQP_GROUP_HAS) UAVQP_GROUP8_PAIRS3(UAVQP_GROUP_HAS)
#undef UAVQP_GROUP_HAS
    return false;
}
// the same lists for host code without the HIP runtime (tests): is there a group kernel for (r, M) at this tile?
static inline bool uavqp_twisted_group_exists(int r, int M, int tile) {
#define UAVQP_GROUP_HAS(R_, M_) if (r == R_ && M == M_) return true;
    if (tile == 4) { UAVQP_GROUP_PAIRS4_T4(UAVQP_GROUP_HAS) UAVQP_GROUP_PAIRS3_T4(UAVQP_GROUP_HAS) }
    if (tile == 8) { UAVQP_GROUP_PAIRS4_T8(UAVQP_GROUP_HAS) UAVQP_GROUP_PAIRS3_T8(UAVQP_GROUP_HAS) }
#undef UAVQP_GROUP_HAS
    return false;
}

// ---- qp_core_kernels.h / qp_generic2.h: the ragged solvers
#define UAVQP_GENERIC_R(R_)                                                                \
    UAVQP_INST __global__ void uavqp::solve_generic2_kernel<R_, true>(uavqp::BatchArgs);      \
    UAVQP_INST __global__ void uavqp::solve_generic2_kernel<R_, false>(uavqp::BatchArgs);     \
    UAVQP_INST __global__ void uavqp::solve_generic_kernel<R_, true, 3>(uavqp::BatchArgs);    \
    UAVQP_INST __global__ void uavqp::solve_generic_kernel<R_, false, 3>(uavqp::BatchArgs);   \
    UAVQP_INST __global__ void uavqp::solve_generic_kernel<R_, true, 1>(uavqp::BatchArgs);    \
    UAVQP_INST __global__ void uavqp::solve_generic_kernel<R_, false, 1>(uavqp::BatchArgs);
#define UAVQP_INSTANCES_GENERIC UAVQP_GENERIC_R(3) UAVQP_GENERIC_R(4)

// ---- qp_corridor.h: the exact corridor solve
#define UAVQP_INSTANCES_CORRIDOR                                                                                      \
    UAVQP_INST __global__ void uavqp::corridor_solve_kernel<3, true, UAVQP_CORRIDOR_WAVES_PER_CU>(uavqp::CorridorArgs);  \
    UAVQP_INST __global__ void uavqp::corridor_solve_kernel<3, false, UAVQP_CORRIDOR_WAVES_PER_CU>(uavqp::CorridorArgs); \
    UAVQP_INST __global__ void uavqp::corridor_solve_kernel<4, true, UAVQP_CORRIDOR_WAVES_PER_CU>(uavqp::CorridorArgs);  \
    UAVQP_INST __global__ void uavqp::corridor_solve_kernel<4, false, UAVQP_CORRIDOR_WAVES_PER_CU>(uavqp::CorridorArgs); \
    UAVQP_INST __global__ void uavqp::corridor_solve_kernel<4, true, 2>(uavqp::CorridorArgs);                            \
    UAVQP_INST __global__ void uavqp::corridor_solve_kernel<4, false, 2>(uavqp::CorridorArgs);

// ---- qp_corridor_dual.h: the position-space dual preludes
#define UAVQP_CORRIDOR_DUAL_R(R_)                                                                             \
    UAVQP_INST __global__ void uavqp::corridor_dual_kernel<R_, 8, 16>(uavqp::CorridorArgs, int, int, int);       \
    UAVQP_INST __global__ void uavqp::corridor_dual_kernel<R_, 16, 24>(uavqp::CorridorArgs, int, int, int);      \
    UAVQP_INST __global__ void uavqp::corridor_dual_kernel<R_, 16, 32>(uavqp::CorridorArgs, int, int, int);      \
    UAVQP_INST __global__ void uavqp::corridor_dual_mixed_kernel<R_>(uavqp::CorridorArgs, int, int);             \
    UAVQP_INST __global__ void uavqp::corridor_dual_wave_kernel<R_>(uavqp::CorridorArgs, int);                   \
    UAVQP_INST __global__ void uavqp::corridor_dual_wave2_kernel<R_>(uavqp::CorridorArgs, int);
#define UAVQP_INSTANCES_CORRIDOR_DUAL UAVQP_CORRIDOR_DUAL_R(3) UAVQP_CORRIDOR_DUAL_R(4)

// ---- qp_rows.h / qp_rows2.h: the general-rows solvers
#define UAVQP_ROWS_RK(R_, K_)                                                                  \
    UAVQP_INST __global__ void uavqp::rows_solve_kernel<R_, K_>(uavqp::RowsArgs);                 \
    UAVQP_INST __global__ void uavqp::rows_pair_kernel<R_, K_, true, false, false>(uavqp::Rows2Args);    \
    UAVQP_INST __global__ void uavqp::rows_pair_kernel<R_, K_, true, false, true>(uavqp::Rows2Args);     \
    UAVQP_INST __global__ void uavqp::rows_pair_kernel<R_, K_, true, true, false>(uavqp::Rows2Args);     \
    UAVQP_INST __global__ void uavqp::rows_pair_kernel<R_, K_, false, false, false>(uavqp::Rows2Args);   \
    UAVQP_INST __global__ void uavqp::rows_pair_kernel<R_, K_, false, false, true>(uavqp::Rows2Args);    \
    UAVQP_INST __global__ void uavqp::rows_pair_kernel<R_, K_, false, true, false>(uavqp::Rows2Args);
// (one translation unit per (R, K): k_rows31.hip ... k_rows42.hip -- five register-heavy kernels each)
#define UAVQP_INSTANCES_ROWS31 UAVQP_ROWS_RK(3, 1)
#define UAVQP_INSTANCES_ROWS32 UAVQP_ROWS_RK(3, 2)
#define UAVQP_INSTANCES_ROWS41 UAVQP_ROWS_RK(4, 1)
#define UAVQP_INSTANCES_ROWS42 UAVQP_ROWS_RK(4, 2)

// ---- qp_rows_dual.h: the starting set of the rows solve
#define UAVQP_ROWS_DUAL_RK(R_, K_) UAVQP_INST __global__ void uavqp::rows_dual_kernel<R_, K_>(uavqp::RowsDualArgs, int);
#define UAVQP_INSTANCES_ROWS_DUAL UAVQP_ROWS_DUAL_RK(3, 1) UAVQP_ROWS_DUAL_RK(3, 2) UAVQP_ROWS_DUAL_RK(4, 1) UAVQP_ROWS_DUAL_RK(4, 2)

// ---- obstacle_grid.h: boxes from the cloud, grid collision check
#define UAVQP_CLOUD_R(R_)                                                                 \
    UAVQP_INST __global__ void uavqp::cloud_window_kernel<R_, 2>(uavqp::CloudCorridorArgs);  \
    UAVQP_INST __global__ void uavqp::cloud_corridor_kernel<R_>(uavqp::CloudCorridorArgs);   \
    UAVQP_INST __global__ void uavqp::ellipsoid_grid_kernel<R_>(uavqp::EllipsoidGridArgs);
#define UAVQP_INSTANCES_CLOUD UAVQP_CLOUD_R(3) UAVQP_CLOUD_R(4)

// ---- qp_time_opt.h: cost + time gradient of solved trajectories, the steps of the duration optimiser
#define UAVQP_TIMEOPT_R(R_)                                                               \
    UAVQP_INST __global__ void uavqp::cost_grad_kernel<R_>(uavqp::CostGradArgs);             \
    UAVQP_INST __global__ void uavqp::time_opt_clamp_kernel<R_>(uavqp::TimeOptArgs);         \
    UAVQP_INST __global__ void uavqp::time_opt_step_kernel<R_, true>(uavqp::TimeOptArgs);    \
    UAVQP_INST __global__ void uavqp::time_opt_step_kernel<R_, false>(uavqp::TimeOptArgs);
#define UAVQP_INSTANCES_TIMEOPT UAVQP_TIMEOPT_R(3) UAVQP_TIMEOPT_R(4)

// ---- qp_adjoint.h: backward pass of the equality-constrained solve
#define UAVQP_ADJOINT_R(R_) UAVQP_INST __global__ void uavqp::solve_backward_kernel<R_>(uavqp::AdjointArgs);
#define UAVQP_INSTANCES_ADJOINT UAVQP_ADJOINT_R(3) UAVQP_ADJOINT_R(4)

// ---- qp_limits.h: velocity / acceleration limit penalty with its gradients, the steps of the limit-aware duration optimiser
#define UAVQP_LIMITS_R(R_)                                                                      \
    UAVQP_INST __global__ void uavqp::limit_penalty_kernel<R_>(uavqp::LimitArgs);                  \
    UAVQP_INST __global__ void uavqp::time_opt_step_kernel<R_, true, true>(uavqp::TimeOptArgs);    \
    UAVQP_INST __global__ void uavqp::time_opt_step_kernel<R_, false, true>(uavqp::TimeOptArgs);
#define UAVQP_INSTANCES_LIMITS UAVQP_LIMITS_R(3) UAVQP_LIMITS_R(4)

// ---- qp_esdf.h: distance field passes and the clearance penalty (its plain kernels are defined in k_esdf.hip alone, declared elsewhere)
#define UAVQP_INSTANCES_ESDF                                                                       \
    UAVQP_INST __global__ void uavqp::esdf_axis_kernel<false>(uavqp::EsdfArgs, int, int, int, int, int); \
    UAVQP_INST __global__ void uavqp::esdf_axis_kernel<true>(uavqp::EsdfArgs, int, int, int, int, int);  \
    UAVQP_INST __global__ void uavqp::clearance_penalty_kernel<3>(uavqp::ClearanceArgs);              \
    UAVQP_INST __global__ void uavqp::clearance_penalty_kernel<4>(uavqp::ClearanceArgs);

// ---- qp_waypoint_opt.h: waypoint gradient of the control cost, the steps of the waypoint optimiser
#define UAVQP_WPOPT_R(R_)                                                                          \
    UAVQP_INST __global__ void uavqp::cost_waypoint_grad_kernel<R_>(uavqp::WaypointGradArgs);         \
    UAVQP_INST __global__ void uavqp::waypoint_opt_step_kernel<R_, true>(uavqp::WaypointOptArgs);     \
    UAVQP_INST __global__ void uavqp::waypoint_opt_step_kernel<R_, false>(uavqp::WaypointOptArgs);
#define UAVQP_INSTANCES_WPOPT UAVQP_WPOPT_R(3) UAVQP_WPOPT_R(4)

// ---- qp_spacetime.h: the fused flight penalty (limits + clearance in one launch), the steps of the joint waypoint / duration optimiser
#define UAVQP_SPACETIME_R(R_)                                                                   \
    UAVQP_INST __global__ void uavqp::flight_penalty_kernel<R_>(uavqp::FlightArgs);                \
    UAVQP_INST __global__ void uavqp::spacetime_step_kernel<R_, true>(uavqp::SpacetimeArgs);       \
    UAVQP_INST __global__ void uavqp::spacetime_step_kernel<R_, false>(uavqp::SpacetimeArgs);
#define UAVQP_INSTANCES_SPACETIME UAVQP_SPACETIME_R(3) UAVQP_SPACETIME_R(4)

// ---- qp_spacetime_lbfgs.h: the step of the joint optimiser with limited-memory BFGS directions
#define UAVQP_SPACETIME_LBFGS_R(R_)                                                                        \
    UAVQP_INST __global__ void uavqp::spacetime_lbfgs_step_kernel<R_, true>(uavqp::SpacetimeLbfgsArgs);       \
    UAVQP_INST __global__ void uavqp::spacetime_lbfgs_step_kernel<R_, false>(uavqp::SpacetimeLbfgsArgs);
#define UAVQP_INSTANCES_SPACETIME_LBFGS UAVQP_SPACETIME_LBFGS_R(3) UAVQP_SPACETIME_LBFGS_R(4)

// ---- qp_swarm.h: the separation penalty between the vehicles of a swarm on a shared clock
#define UAVQP_SWARM_R(R_) UAVQP_INST __global__ void uavqp::swarm_penalty_kernel<R_>(uavqp::SwarmArgs);
#define UAVQP_INSTANCES_SWARM UAVQP_SWARM_R(3) UAVQP_SWARM_R(4)

// ---- qp_swarm_opt.h: the per-swarm step of the swarm optimiser, and the swarm penalty that ADDS its gradients to the flight penalty's
#define UAVQP_SWARM_OPT_R(R_)                                                                  \
    UAVQP_INST __global__ void uavqp::swarm_penalty_kernel<R_, true>(uavqp::SwarmArgs);           \
    UAVQP_INST __global__ void uavqp::swarm_step_kernel<R_, true>(uavqp::SwarmOptArgs);           \
    UAVQP_INST __global__ void uavqp::swarm_step_kernel<R_, false>(uavqp::SwarmOptArgs);
#define UAVQP_INSTANCES_SWARM_OPT UAVQP_SWARM_OPT_R(3) UAVQP_SWARM_OPT_R(4)

// ---- qp_attitude.h: thrust / tilt / body-rate penalty with its gradients, and the variant that ADDS them to the flight penalty's
#define UAVQP_ATTITUDE_R(R_)                                                                     \
    UAVQP_INST __global__ void uavqp::attitude_penalty_kernel<R_, false>(uavqp::AttitudeArgs);      \
    UAVQP_INST __global__ void uavqp::attitude_penalty_kernel<R_, true>(uavqp::AttitudeArgs);
#define UAVQP_INSTANCES_ATTITUDE UAVQP_ATTITUDE_R(3) UAVQP_ATTITUDE_R(4)

// ---- qp_moving.h: penalty against moving obstacle tracks with its gradients, and the variant that ADDS them to the flight penalty's
#define UAVQP_MOVING_R(R_)                                                                   \
    UAVQP_INST __global__ void uavqp::moving_penalty_kernel<R_, false>(uavqp::MovingArgs);      \
    UAVQP_INST __global__ void uavqp::moving_penalty_kernel<R_, true>(uavqp::MovingArgs);
#define UAVQP_INSTANCES_MOVING UAVQP_MOVING_R(3) UAVQP_MOVING_R(4)

// ---- qp_envelope.h: certified bounds of position, velocity, acceleration, jerk, thrust and tilt over whole segments
#define UAVQP_ENVELOPE_R(R_) UAVQP_INST __global__ void uavqp::envelope_kernel<R_>(uavqp::EnvelopeArgs);
#define UAVQP_INSTANCES_ENVELOPE UAVQP_ENVELOPE_R(3) UAVQP_ENVELOPE_R(4)

// ---- qp_clearance_cert.h: certified clearance of whole segments against the distance field's integer squared distances
#define UAVQP_CLEARANCE_CERT_R(R_) UAVQP_INST __global__ void uavqp::clearance_cert_kernel<R_>(uavqp::ClearanceCertArgs);
#define UAVQP_INSTANCES_CLEARANCE_CERT UAVQP_CLEARANCE_CERT_R(3) UAVQP_CLEARANCE_CERT_R(4)

// ---- qp_separation_cert.h: certified separation between the vehicles of a swarm over a whole clock window
#define UAVQP_SEPARATION_CERT_R(R_) UAVQP_INST __global__ void uavqp::separation_cert_kernel<R_>(uavqp::SeparationCertArgs);
#define UAVQP_INSTANCES_SEPARATION_CERT UAVQP_SEPARATION_CERT_R(3) UAVQP_SEPARATION_CERT_R(4)

// ---- qp_moving_cert.h: certified gap of whole segments to moving obstacle tracks
#define UAVQP_MOVING_CERT_R(R_) UAVQP_INST __global__ void uavqp::moving_cert_kernel<R_>(uavqp::MovingCertArgs);
#define UAVQP_INSTANCES_MOVING_CERT UAVQP_MOVING_CERT_R(3) UAVQP_MOVING_CERT_R(4)
