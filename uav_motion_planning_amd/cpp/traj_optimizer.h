// TrajOptimizer -- batch facade with the method names BASELINE.json's north star asks for
// (setWaypoints / setTimeAllocation / solve / getPolyCoeff).  The reference has no such class
// (its only optimiser is traj_optimization::MinimumControl); this is the batch-oriented
// entry a planner would call once per replanning cycle for all candidate trajectories and all 3 axes.
// Header-only, no Eigen: plain pointers over the C ABI (include/uavqp.h).
#ifndef UAVQP_TRAJ_OPTIMIZER_H_
#define UAVQP_TRAJ_OPTIMIZER_H_

#include <algorithm>
#include <cstdint>
#include <iostream>
#include <vector>

#include "../../include/uavqp.h"

// The sharded (multi-GPU) entry keeps its buffers on the device and therefore needs the HIP runtime API for allocation and the
// host <-> device copies at its two ends; everything else here is plain C ABI.  A planner that runs one process (or thread) per GPU
// has it anyway.
#if defined(__has_include)
#if __has_include(<hip/hip_runtime_api.h>)
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>
#define UAVQP_TRAJ_OPTIMIZER_HAS_HIP 1
#endif
#endif

namespace traj_optimization {

// How solvePipeline() repairs a trajectory the final collision check flags (include/uavqp.h): Boxes shrinks its knot boxes towards the
// waypoints (last round: the waypoint equalities); Rows adds position rows inside the colliding segments and keeps the knot boxes.
enum class PipelineRepair { Boxes, Rows };

class TrajOptimizer {
  public:
    explicit TrajOptimizer(int order = 4, int device = 0) : order_(order), device_(device) {}
    ~TrajOptimizer() { if (ctx_) uavqp_destroy(ctx_); }
    TrajOptimizer(const TrajOptimizer&) = delete;
    TrajOptimizer& operator=(const TrajOptimizer&) = delete;

    // xyz: [sum_b n_waypoints_b][3]; wp_offsets[n_traj+1]: first waypoint row of each trajectory
    // (what a list of A* / kino-A* / RRT* paths flattens to).
    void setWaypoints(const double* xyz, const int32_t* wp_offsets, int n_traj) {
        n_traj_ = n_traj;
        seg_offsets_.resize(n_traj + 1);
        for (int b = 0; b <= n_traj; ++b) seg_offsets_[b] = wp_offsets[b] - b;  // M_b = n_waypoints_b - 1
        wp_.assign(xyz, xyz + 3 * static_cast<size_t>(wp_offsets[n_traj]));
    }
    // T: [sum_b M_b] segment durations in trajectory order.
    void setTimeAllocation(const double* T) { T_.assign(T, T + (n_traj_ > 0 ? seg_offsets_[n_traj_] : 0)); }
    // bc: [n_traj][2][order-1][3] = [start|end][vel, acc(, jerk)][xyz]; default all zero.
    void setBoundary(const double* bc) { bc_.assign(bc, bc + static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3); }
    // Optional corridor (north-star extension): boxes lo <= p <= hi, [sum_b n_waypoints_b][3] like xyz, replace the
    // interior-waypoint equalities; first/last rows of a trajectory are ignored.  nullptr restores the equalities.
    void setCorridor(const double* lo, const double* hi) {
        lo_.clear();
        hi_.clear();
        if (lo && hi) {
            lo_.assign(lo, lo + wp_.size());
            hi_.assign(hi, hi + wp_.size());
        }
    }

    // Optional general inequality rows (north-star extension; what the reference's solver interface accepts,
    // minimum_control.cpp:146-147,164-180): per segment and slot j < rows_per_segment (1 or 2) a row
    // lo <= p^(deriv)(tau * T_segment) <= hi per axis.  tau / deriv: [sum_b M_b][K], lo / hi: [sum_b M_b][K][3]; deriv < 0 = unused
    // slot.  Needs setTimeAllocation first (sizes).  rows_per_segment = 0 removes them.
    void setRows(int rows_per_segment, const double* tau, const int32_t* deriv, const double* lo, const double* hi) {
        rows_k_ = rows_per_segment;
        if (rows_k_ <= 0 || !tau || !deriv || !lo || !hi) { rows_k_ = 0; return; }   // (null arrays: no rows, never a wild read)
        const size_t n = T_.size() * static_cast<size_t>(rows_k_);
        row_tau_.assign(tau, tau + n);
        row_deriv_.assign(deriv, deriv + n);
        row_lo_.assign(lo, lo + 3 * n);
        row_hi_.assign(hi, hi + 3 * n);
    }

    // Solver settings (include/uavqp.h: the reference's warm_start / eps_prim_inf / max_iter, minimum_control.cpp:160-162, and the
    // library's own knobs).  Applied to the context now, or when it is created.
    bool setSettings(const uavqp_settings& st) {
        settings_ = st;
        have_settings_ = true;
        return !ctx_ || uavqp_set_settings(ctx_, &settings_) == UAVQP_OK;
    }

    bool solve() {
        if (n_traj_ <= 0 || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_])) return false;
        if (!rowsMatchBatch() || !corridorMatchesBatch()) {   // rows / boxes installed for another batch size: refuse, never read past them
            std::cout << "solver solve failed! (rows or corridor arrays do not match the current batch)" << std::endl;
            return false;
        }
        if (!ensureContext()) return false;
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        coef_.assign(static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_], 0.0);
        status_.assign(n_traj_, 0);
        int rc;
        if (rows_k_ > 0)
            rc = uavqp_solve_rows_batch_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(),
                                             lo_.empty() ? nullptr : lo_.data(), lo_.empty() ? nullptr : hi_.data(), rows_k_, row_tau_.data(),
                                             row_deriv_.data(), row_lo_.data(), row_hi_.data(), coef_.data(), status_.data(), nullptr);
        else if (lo_.empty())
            rc = uavqp_solve_batch_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), coef_.data(), status_.data());
        else
            rc = uavqp_solve_corridor_batch_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(),
                                                 lo_.data(), hi_.data(), coef_.data(), status_.data(), nullptr);
        if (rc != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        for (int32_t s : status_) if (s != UAVQP_SOLVED) return false;
        return true;
    }
    // Flat coefficients: trajectory b starts at 3*2r*segOffset(b), layout [axis][segment][2r], ascending powers.
    const double* getPolyCoeff() const { return coef_.data(); }
    const double* getPolyCoeff(int traj, int axis) const {
        const int M = seg_offsets_[traj + 1] - seg_offsets_[traj];
        return coef_.data() + static_cast<size_t>(3) * 2 * order_ * seg_offsets_[traj] + static_cast<size_t>(axis) * 2 * order_ * M;
    }
    int segOffset(int traj) const { return seg_offsets_[traj]; }
    const std::vector<int32_t>& status() const { return status_; }

    // Optimisation of the time allocation (include/uavqp.h uavqp_time_optimize_host; the reference's equality rows only: false when a
    // corridor or rows are set): minimises, per trajectory, cost + time_weight * sum T over the durations.  On return timeAllocation() = the
    // optimised durations, getPolyCoeff() = the solve at them, objective() = [n_traj][2] f at the start / at the result, acceptedTrials() per
    // trajectory.  params: null = uavqp_default_time_opt_params; time_weight > 0 overrides its weight.
    bool optimizeTime(double time_weight = 0.0, const uavqp_time_opt_params* params = nullptr) {
        if (n_traj_ <= 0 || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_])) return false;
        if (!lo_.empty() || rows_k_ > 0) {
            std::cout << "solver solve failed! (optimizeTime: corridor and general-rows problems are out of scope)" << std::endl;
            return false;
        }
        if (!ensureContext()) return false;
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        uavqp_time_opt_params pp;
        if (params) pp = *params; else uavqp_default_time_opt_params(&pp);
        if (time_weight > 0.0) pp.time_weight = time_weight;
        coef_.assign(static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_], 0.0);
        status_.assign(n_traj_, 0);
        objective_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        accepted_.assign(n_traj_, 0);
        const int rc = uavqp_time_optimize_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), &pp,
                                                coef_.data(), status_.data(), objective_.data(), accepted_.data());
        if (rc != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        for (int32_t s : status_) if (s != UAVQP_SOLVED) return false;
        return true;
    }
    // The same with the soft velocity / acceleration limit penalty inside the objective (uavqp_time_optimize_limits_host): objective()
    // includes the penalty, peak() = [n_traj][2] sampled |v| / v_max, |a| / a_max at the result.  The penalty is soft: a peak may end
    // above 1 (include/uavqp.h); uavqp_time_reallocate_device afterwards is the hard guarantee.
    bool optimizeTime(const uavqp_limit_params& limits, double time_weight = 0.0, const uavqp_time_opt_params* params = nullptr) {
        if (n_traj_ <= 0 || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_])) return false;
        if (!lo_.empty() || rows_k_ > 0) {
            std::cout << "solver solve failed! (optimizeTime: corridor and general-rows problems are out of scope)" << std::endl;
            return false;
        }
        if (!ensureContext()) return false;
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        uavqp_time_opt_params pp;
        if (params) pp = *params; else uavqp_default_time_opt_params(&pp);
        if (time_weight > 0.0) pp.time_weight = time_weight;
        coef_.assign(static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_], 0.0);
        status_.assign(n_traj_, 0);
        objective_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        accepted_.assign(n_traj_, 0);
        peak_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        const int rc = uavqp_time_optimize_limits_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), &pp,
                                                       coef_.data(), status_.data(), objective_.data(), accepted_.data(), &limits, peak_.data());
        if (rc != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        for (int32_t s : status_) if (s != UAVQP_SOLVED) return false;
        return true;
    }
    const std::vector<double>& peak() const { return peak_; }
    // Limit penalty per trajectory of the stored coefficients at the stored durations (after solve() or optimizeTime();
    // uavqp_limit_penalty_host).  A trajectory that did not solve carries zero.  Empty on failure.
    std::vector<double> getLimitPenalty(const uavqp_limit_params& limits) {
        std::vector<double> phi;
        if (n_traj_ <= 0 || !ctx_ || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]) ||
            coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || status_.size() != static_cast<size_t>(n_traj_))
            return phi;
        phi.assign(n_traj_, 0.0);
        if (uavqp_limit_penalty_host(ctx_, order_, n_traj_, 0, seg_offsets_.data(), T_.data(), coef_.data(), status_.data(), &limits, phi.data(),
                                     nullptr, nullptr, nullptr) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            phi.clear();
        }
        return phi;
    }
    // Which trajectories fly together: swarm g is the trajectories group_offsets[g] .. group_offsets[g + 1] (null: the whole batch is one
    // swarm); start_times [n_traj]: when each departs on its swarm's clock (null: all at 0).  After setWaypoints (sizes).
    void setSwarm(const int32_t* group_offsets, int n_groups, const double* start_times) {
        groups_.clear();
        start_.clear();
        if (group_offsets && n_groups >= 0) groups_.assign(group_offsets, group_offsets + n_groups + 1);
        if (start_times) start_.assign(start_times, start_times + n_traj_);
    }
    // Separation penalty per swarm between the vehicles set with setSwarm, at the stored coefficients and durations (after solve() or
    // optimizeTime(); uavqp_swarm_penalty_host).  min_sep, when given, receives the smallest sampled separation per trajectory.  A
    // trajectory that did not solve is left out of every pair.  Empty on failure.
    std::vector<double> getSwarmPenalty(const uavqp_swarm_params& params, std::vector<double>* min_sep = nullptr) {
        std::vector<double> phi;
        if (n_traj_ <= 0 || !ctx_ || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]) ||
            coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || status_.size() != static_cast<size_t>(n_traj_) ||
            (!start_.empty() && start_.size() != static_cast<size_t>(n_traj_)))
            return phi;
        const int n_groups = groups_.empty() ? 1 : static_cast<int>(groups_.size()) - 1;
        phi.assign(n_groups, 0.0);
        if (min_sep) min_sep->assign(n_traj_, 0.0);
        if (uavqp_swarm_penalty_host(ctx_, order_, n_traj_, 0, seg_offsets_.data(), T_.data(), coef_.data(), status_.data(), n_groups,
                                     groups_.empty() ? nullptr : groups_.data(), start_.empty() ? nullptr : start_.data(), &params, phi.data(),
                                     nullptr, nullptr, nullptr, min_sep ? min_sep->data() : nullptr) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            phi.clear();
        }
        return phi;
    }
    // Certified separation between the vehicles of each swarm set with setSwarm, at the stored coefficients, durations and departures, for
    // EVERY t of the clock window of `params` (after solve() or optimizeSwarm(); uavqp_separation_certificate_host): the hard test that
    // the sampled min_sep is not.  Returns the verdict word per trajectory (UAVQP_SEPARATION_CERTIFIED: at least d_req from every partner
    // for ALL t of the window, UAVQP_SEPARATION_VIOLATED: less at the witness, neither: undecided; UAVQP_SEPARATION_MOVING: still under way
    // at the end of the window) and fills separationLower() / separationUpper() [n_traj], separationWhere() [n_traj][4] ({partner of lower,
    // leaf of lower, partner of upper, witness index of upper}) and separationGroupVerdict() [n_groups].  Empty on failure.
    std::vector<int32_t> getSeparationCertificate(const uavqp_separation_params& params) {
        std::vector<int32_t> verdict;
        if (n_traj_ <= 0 || !ctx_ || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]) ||
            coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || status_.size() != static_cast<size_t>(n_traj_) ||
            (!start_.empty() && start_.size() != static_cast<size_t>(n_traj_)))
            return verdict;
        const int n_groups = groups_.empty() ? 1 : static_cast<int>(groups_.size()) - 1;
        verdict.assign(n_traj_, 0);
        separation_lower_.assign(n_traj_, 0.0);
        separation_upper_.assign(n_traj_, 0.0);
        separation_where_.assign(static_cast<size_t>(4) * n_traj_, 0);
        separation_group_verdict_.assign(n_groups, 0);
        if (uavqp_separation_certificate_host(ctx_, order_, n_traj_, 0, seg_offsets_.data(), T_.data(), coef_.data(), status_.data(), n_groups,
                                              groups_.empty() ? nullptr : groups_.data(), start_.empty() ? nullptr : start_.data(), &params,
                                              separation_lower_.data(), separation_upper_.data(), separation_where_.data(), verdict.data(),
                                              separation_group_verdict_.data()) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            verdict.clear();
        }
        return verdict;
    }
    const std::vector<double>& separationLower() const { return separation_lower_; }
    const std::vector<double>& separationUpper() const { return separation_upper_; }
    const std::vector<int32_t>& separationWhere() const { return separation_where_; }
    const std::vector<int32_t>& separationGroupVerdict() const { return separation_group_verdict_; }
    // Clearance penalty per trajectory of the stored coefficients at the stored durations against a distance field (uavqp::EsdfMap of
    // cpp/esdf_map.h, built on context() and updated; uavqp_clearance_penalty_host).  min_dist / outside, when given, receive the smallest
    // sampled distance and the count of samples outside the map per trajectory.  A trajectory that did not solve carries zero.  Empty on failure.
    template <class Map>
    std::vector<double> getClearancePenalty(const Map& map, const uavqp_clearance_params& params, std::vector<double>* min_dist = nullptr,
                                            std::vector<int32_t>* outside = nullptr) {
        std::vector<double> phi;
        if (n_traj_ <= 0 || !ctx_ || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]) ||
            coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || status_.size() != static_cast<size_t>(n_traj_))
            return phi;
        phi.assign(n_traj_, 0.0);
        if (min_dist) min_dist->assign(n_traj_, 0.0);
        if (outside) outside->assign(n_traj_, 0);
        if (uavqp_clearance_penalty_host(ctx_, order_, n_traj_, 0, seg_offsets_.data(), T_.data(), coef_.data(), status_.data(), map.handle(), &params,
                                         phi.data(), nullptr, nullptr, min_dist ? min_dist->data() : nullptr,
                                         outside ? outside->data() : nullptr) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            phi.clear();
        }
        return phi;
    }
    // Optimisation of the interior waypoints against a distance field (include/uavqp.h uavqp_waypoint_optimize_host; the reference's
    // equality rows only: false when a corridor or rows are set): minimises, per trajectory, smooth_weight * cost + clearance penalty over
    // the interior waypoints inside a box of half edge max_move around the start.  map: a uavqp::EsdfMap of cpp/esdf_map.h built on
    // context() and updated.  On return waypoints() = the optimised waypoints (end knots untouched), getPolyCoeff() = the solve at them,
    // objective() = [n_traj][2] f at the start / at the result, acceptedTrials() per trajectory, minDist() / outsideSamples() the penalty's
    // diagnostics at the result.  params: null = uavqp_default_waypoint_opt_params; smooth_weight >= 0 overrides its weight.  The penalty is
    // soft and the result a local minimum: uavqp_ellipsoid_check_* afterwards remains the hard test.
    template <class Map>
    bool optimizeWaypoints(const Map& map, const uavqp_clearance_params& clearance, double smooth_weight = -1.0,
                           const uavqp_waypoint_opt_params* params = nullptr) {
        if (n_traj_ <= 0 || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_])) return false;
        if (!lo_.empty() || rows_k_ > 0) {
            std::cout << "solver solve failed! (optimizeWaypoints: corridor and general-rows problems are out of scope)" << std::endl;
            return false;
        }
        if (!ensureContext()) return false;
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        uavqp_waypoint_opt_params pp;
        if (params) pp = *params; else uavqp_default_waypoint_opt_params(&pp);
        if (smooth_weight >= 0.0) pp.smooth_weight = smooth_weight;
        coef_.assign(static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_], 0.0);
        status_.assign(n_traj_, 0);
        objective_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        accepted_.assign(n_traj_, 0);
        min_dist_.assign(n_traj_, 0.0);
        outside_.assign(n_traj_, 0);
        const int rc = uavqp_waypoint_optimize_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), map.handle(),
                                                    &clearance, &pp, coef_.data(), status_.data(), objective_.data(), accepted_.data(),
                                                    min_dist_.data(), outside_.data());
        if (rc != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        for (int32_t s : status_) if (s != UAVQP_SOLVED) return false;
        return true;
    }
    // Joint optimisation of the interior waypoints AND the durations under both penalties (include/uavqp.h uavqp_spacetime_optimize_host;
    // the reference's equality rows only: false when a corridor or rows are set): minimises, per trajectory, smooth_weight * cost +
    // time_weight * sum T + limit penalty + clearance penalty against `map` (a uavqp::EsdfMap of cpp/esdf_map.h built on context() and
    // updated).  On return waypoints() / timeAllocation() = the optimised point, getPolyCoeff() = the solve at it, objective() =
    // [n_traj][2] f at the start / at the result, acceptedTrials() per trajectory, peak() / minDist() / outsideSamples() the penalties'
    // diagnostics at the result.  params: null = uavqp_default_spacetime_params.  Both penalties are soft and the result a local minimum:
    // uavqp_time_reallocate_device and uavqp_ellipsoid_check_* afterwards remain the hard tests.
    template <class Map>
    bool optimizeTrajectory(const Map& map, const uavqp_limit_params& limits, const uavqp_clearance_params& clearance,
                            const uavqp_spacetime_params* params = nullptr) {
        if (n_traj_ <= 0 || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_])) return false;
        if (!lo_.empty() || rows_k_ > 0) {
            std::cout << "solver solve failed! (optimizeTrajectory: corridor and general-rows problems are out of scope)" << std::endl;
            return false;
        }
        if (!ensureContext()) return false;
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        uavqp_spacetime_params pp;
        if (params) pp = *params; else uavqp_default_spacetime_params(&pp);
        coef_.assign(static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_], 0.0);
        status_.assign(n_traj_, 0);
        objective_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        accepted_.assign(n_traj_, 0);
        peak_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        min_dist_.assign(n_traj_, 0.0);
        outside_.assign(n_traj_, 0);
        const int rc = uavqp_spacetime_optimize_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), map.handle(),
                                                     &limits, &clearance, &pp, coef_.data(), status_.data(), objective_.data(), accepted_.data(),
                                                     peak_.data(), min_dist_.data(), outside_.data());
        if (rc != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        for (int32_t s : status_) if (s != UAVQP_SOLVED) return false;
        return true;
    }
    // The same with limited-memory BFGS directions kept per trajectory on the device (include/uavqp.h uavqp_spacetime_lbfgs_host): the same
    // objective and bounds, the same members filled, fewer trials to the same objective.  params: null =
    // uavqp_default_spacetime_lbfgs_params.  (Its own name and not an overload: with both parameter pointers defaulted a call without one
    // would be ambiguous.)
    template <class Map>
    bool optimizeTrajectoryLbfgs(const Map& map, const uavqp_limit_params& limits, const uavqp_clearance_params& clearance,
                                 const uavqp_spacetime_lbfgs_params* params = nullptr) {
        if (n_traj_ <= 0 || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_])) return false;
        if (!lo_.empty() || rows_k_ > 0) {
            std::cout << "solver solve failed! (optimizeTrajectoryLbfgs: corridor and general-rows problems are out of scope)" << std::endl;
            return false;
        }
        if (!ensureContext()) return false;
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        uavqp_spacetime_lbfgs_params pp;
        if (params) pp = *params; else uavqp_default_spacetime_lbfgs_params(&pp);
        coef_.assign(static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_], 0.0);
        status_.assign(n_traj_, 0);
        objective_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        accepted_.assign(n_traj_, 0);
        peak_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        min_dist_.assign(n_traj_, 0.0);
        outside_.assign(n_traj_, 0);
        const int rc = uavqp_spacetime_lbfgs_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), map.handle(),
                                                  &limits, &clearance, &pp, coef_.data(), status_.data(), objective_.data(), accepted_.data(),
                                                  peak_.data(), min_dist_.data(), outside_.data());
        if (rc != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        for (int32_t s : status_) if (s != UAVQP_SOLVED) return false;
        return true;
    }
    // optimizeTrajectoryLbfgs with the attitude penalty -- specific thrust, tilt and body rate of the vehicle -- inside the objective
    // (include/uavqp.h uavqp_attitude_optimize_host): the same bounds, the same members filled, and attitudePeak() [n_traj][4] = largest and
    // smallest specific thrust (m/s^2), largest tilt (rad), largest body rate (rad/s) sampled at the result.  The penalty is soft:
    // attitudePeak() is the check afterwards.  params: null = uavqp_default_spacetime_lbfgs_params.
    template <class Map>
    bool optimizeTrajectoryAttitude(const Map& map, const uavqp_limit_params& limits, const uavqp_clearance_params& clearance,
                                    const uavqp_attitude_params& attitude, const uavqp_spacetime_lbfgs_params* params = nullptr) {
        if (n_traj_ <= 0 || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_])) return false;
        if (!lo_.empty() || rows_k_ > 0) {
            std::cout << "solver solve failed! (optimizeTrajectoryAttitude: corridor and general-rows problems are out of scope)" << std::endl;
            return false;
        }
        if (!ensureContext()) return false;
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        uavqp_spacetime_lbfgs_params pp;
        if (params) pp = *params; else uavqp_default_spacetime_lbfgs_params(&pp);
        coef_.assign(static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_], 0.0);
        status_.assign(n_traj_, 0);
        objective_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        accepted_.assign(n_traj_, 0);
        peak_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        min_dist_.assign(n_traj_, 0.0);
        outside_.assign(n_traj_, 0);
        attitude_peak_.assign(static_cast<size_t>(4) * n_traj_, 0.0);
        const int rc = uavqp_attitude_optimize_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), map.handle(),
                                                    &limits, &clearance, &attitude, &pp, coef_.data(), status_.data(), objective_.data(),
                                                    accepted_.data(), peak_.data(), min_dist_.data(), outside_.data(), attitude_peak_.data());
        if (rc != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        for (int32_t s : status_) if (s != UAVQP_SOLVED) return false;
        return true;
    }
    // Attitude penalty per trajectory of the stored coefficients at the stored durations (after solve() or an optimiser;
    // uavqp_attitude_penalty_host); fills attitudePeak().  A trajectory that did not solve carries zero.  Empty on failure.
    std::vector<double> getAttitudePenalty(const uavqp_attitude_params& attitude) {
        std::vector<double> phi;
        if (n_traj_ <= 0 || !ctx_ || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]) ||
            coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || status_.size() != static_cast<size_t>(n_traj_))
            return phi;
        phi.assign(n_traj_, 0.0);
        attitude_peak_.assign(static_cast<size_t>(4) * n_traj_, 0.0);
        if (uavqp_attitude_penalty_host(ctx_, order_, n_traj_, 0, seg_offsets_.data(), T_.data(), coef_.data(), status_.data(), &attitude,
                                        phi.data(), nullptr, nullptr, attitude_peak_.data()) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            phi.clear();
        }
        return phi;
    }
    const std::vector<double>& attitudePeak() const { return attitude_peak_; }
    // The moving obstacles the trajectories avoid (include/uavqp.h uavqp_moving_obstacles, host pointers; the arrays are COPIED): tracks in
    // the library's own format and this optimiser's order -- obstacles.times / coeff / seg_offsets or uniform_segments -- with their
    // departures and radii, the sets, the set each trajectory avoids and the trajectories' own departures.  nullptr removes them.
    // false: the struct is refused (its size, a negative count, a missing array) and nothing is stored.
    bool setMovingObstacles(const uavqp_moving_obstacles* obstacles) {
        moving_ = MovingStore();
        if (!obstacles) return true;
        const uavqp_moving_obstacles& o = *obstacles;
        if (o.struct_size != static_cast<int32_t>(sizeof(uavqp_moving_obstacles)) || o.n_obs < 0 || o.uniform_segments < 0 || o.n_sets < 0) return false;
        if (o.n_obs > 0 && (!o.times || !o.coeff || (o.uniform_segments == 0 && !o.seg_offsets))) return false;
        if (o.n_sets != 1 && (!o.set_offsets || !o.traj_set)) return false;
        if ((o.traj_set || o.traj_start) && n_traj_ <= 0) return false;   // (their length is the batch's: setWaypoints first)
        MovingStore m;
        size_t total = static_cast<size_t>(o.uniform_segments) * o.n_obs;
        if (o.n_obs > 0 && o.uniform_segments == 0) {
            m.seg_offsets.assign(o.seg_offsets, o.seg_offsets + o.n_obs + 1);
            if (m.seg_offsets[o.n_obs] < 0) return false;
            total = static_cast<size_t>(m.seg_offsets[o.n_obs]);
        }
        if (o.n_obs > 0) {
            m.times.assign(o.times, o.times + total);
            m.coeff.assign(o.coeff, o.coeff + static_cast<size_t>(3) * 2 * order_ * total);
            if (o.start) m.start.assign(o.start, o.start + o.n_obs);
            if (o.radius) m.radius.assign(o.radius, o.radius + o.n_obs);
        }
        if (o.set_offsets) m.set_offsets.assign(o.set_offsets, o.set_offsets + o.n_sets + 1);
        if (o.traj_set) m.traj_set.assign(o.traj_set, o.traj_set + n_traj_);
        if (o.traj_start) m.traj_start.assign(o.traj_start, o.traj_start + n_traj_);
        m.n_obs = o.n_obs; m.uniform_segments = o.uniform_segments; m.n_sets = o.n_sets; m.set = true;
        moving_ = m;
        return true;
    }
    // Penalty per trajectory against the obstacles of setMovingObstacles at the stored coefficients and durations (after solve() or an
    // optimiser; uavqp_moving_penalty_host); fills minGap() / nearestObstacle().  A trajectory that did not solve carries zero.  Empty on
    // failure.
    std::vector<double> getMovingPenalty(const uavqp_moving_params& moving) {
        std::vector<double> phi;
        if (!moving_.set || n_traj_ <= 0 || !ctx_ || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]) ||
            coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || status_.size() != static_cast<size_t>(n_traj_))
            return phi;
        phi.assign(n_traj_, 0.0);
        min_gap_.assign(n_traj_, 0.0);
        nearest_.assign(n_traj_, -1);
        const uavqp_moving_obstacles o = moving_.view();
        if (uavqp_moving_penalty_host(ctx_, order_, n_traj_, 0, seg_offsets_.data(), T_.data(), coef_.data(), status_.data(), &o, &moving,
                                      phi.data(), nullptr, nullptr, nullptr, min_gap_.data(), nearest_.data()) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            phi.clear();
        }
        return phi;
    }
    // optimizeTrajectoryAttitude with the penalty against the obstacles of setMovingObstacles inside the objective (include/uavqp.h
    // uavqp_moving_optimize_host): the same bounds, the same members filled, and minGap() / nearestObstacle() at the result.  attitude null:
    // NO attitude term.  The penalty is soft: minGap() is the check afterwards, on the samples.  params: null =
    // uavqp_default_spacetime_lbfgs_params.
    template <class Map>
    bool optimizeTrajectoryMoving(const Map& map, const uavqp_limit_params& limits, const uavqp_clearance_params& clearance,
                                  const uavqp_attitude_params* attitude, const uavqp_moving_params& moving,
                                  const uavqp_spacetime_lbfgs_params* params = nullptr) {
        if (!moving_.set || n_traj_ <= 0 || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_])) return false;
        if (!lo_.empty() || rows_k_ > 0) {
            std::cout << "solver solve failed! (optimizeTrajectoryMoving: corridor and general-rows problems are out of scope)" << std::endl;
            return false;
        }
        if (!ensureContext()) return false;
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        uavqp_spacetime_lbfgs_params pp;
        if (params) pp = *params; else uavqp_default_spacetime_lbfgs_params(&pp);
        coef_.assign(static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_], 0.0);
        status_.assign(n_traj_, 0);
        objective_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        accepted_.assign(n_traj_, 0);
        peak_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        min_dist_.assign(n_traj_, 0.0);
        outside_.assign(n_traj_, 0);
        attitude_peak_.assign(static_cast<size_t>(4) * n_traj_, 0.0);
        min_gap_.assign(n_traj_, 0.0);
        nearest_.assign(n_traj_, -1);
        const uavqp_moving_obstacles o = moving_.view();
        const int rc = uavqp_moving_optimize_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), map.handle(),
                                                  &limits, &clearance, attitude, &o, &moving, &pp, coef_.data(), status_.data(), objective_.data(),
                                                  accepted_.data(), peak_.data(), min_dist_.data(), outside_.data(), attitude_peak_.data(),
                                                  min_gap_.data(), nearest_.data());
        if (rc != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        for (int32_t s : status_) if (s != UAVQP_SOLVED) return false;
        return true;
    }
    const std::vector<double>& minGap() const { return min_gap_; }
    const std::vector<int32_t>& nearestObstacle() const { return nearest_; }
    // Certified gap of every segment to the obstacles of setMovingObstacles, at the stored coefficients and durations, for EVERY t of the
    // segment (after solve() or an optimiser; uavqp_moving_certificate_host): the hard test that the sampled minGap() is not.  Returns the
    // verdict word per trajectory (UAVQP_MOVING_CERT_CERTIFIED: at least d_req from every obstacle's surface for ALL t,
    // UAVQP_MOVING_CERT_VIOLATED: less at the witness, neither: undecided -- raise depth or replan) and fills movingGap() [sum M][2] (lower,
    // upper), movingWhere() [sum M][4] ({obstacle of lower, leaf of lower, obstacle of upper, witness index of upper}), movingPeak()
    // [n_traj][2] and movingSegVerdict() [sum M].  Empty on failure.
    std::vector<int32_t> getMovingCertificate(const uavqp_moving_cert_params& params) {
        std::vector<int32_t> verdict;
        if (!moving_.set || n_traj_ <= 0 || !ctx_ || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]) ||
            coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || status_.size() != static_cast<size_t>(n_traj_))
            return verdict;
        const size_t total = static_cast<size_t>(seg_offsets_[n_traj_]);
        verdict.assign(n_traj_, 0);
        moving_gap_.assign(2 * total, 0.0);
        moving_where_.assign(4 * total, 0);
        moving_peak_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        moving_seg_verdict_.assign(total, 0);
        const uavqp_moving_obstacles o = moving_.view();
        if (uavqp_moving_certificate_host(ctx_, order_, n_traj_, 0, seg_offsets_.data(), T_.data(), coef_.data(), status_.data(), &o, &params,
                                          moving_gap_.data(), moving_where_.data(), moving_peak_.data(), moving_seg_verdict_.data(),
                                          verdict.data()) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            verdict.clear();
        }
        return verdict;
    }
    const std::vector<double>& movingGap() const { return moving_gap_; }
    const std::vector<int32_t>& movingWhere() const { return moving_where_; }
    const std::vector<double>& movingPeak() const { return moving_peak_; }
    const std::vector<int32_t>& movingSegVerdict() const { return moving_seg_verdict_; }
    // Certified bounds of the stored coefficients at the stored durations over WHOLE segments (after solve() or an optimiser;
    // uavqp_envelope_host): the verdict word per trajectory (bit 2k certified for all t, bit 2k + 1 violated, UAVQP_ENVELOPE_* of
    // include/uavqp.h), and envelopeRange() [sum M][4][3][4], envelopeNorm() [sum M][5][4], envelopePeak() [n_traj][5][4],
    // envelopeSegVerdict() [sum M] filled.  box_lo / box_hi: [sum M][3], one box per segment, both or neither (nullptr: off).  A trajectory
    // that did not solve carries zeros.  Empty on failure.
    std::vector<int32_t> getEnvelope(const uavqp_envelope_params& envelope, const double* box_lo = nullptr, const double* box_hi = nullptr) {
        std::vector<int32_t> verdict;
        if (n_traj_ <= 0 || !ctx_ || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]) ||
            coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || status_.size() != static_cast<size_t>(n_traj_))
            return verdict;
        const size_t tot = static_cast<size_t>(seg_offsets_[n_traj_]);
        verdict.assign(n_traj_, 0);
        envelope_range_.assign(48 * tot, 0.0);
        envelope_norm_.assign(20 * tot, 0.0);
        envelope_peak_.assign(static_cast<size_t>(20) * n_traj_, 0.0);
        envelope_seg_verdict_.assign(tot, 0);
        if (uavqp_envelope_host(ctx_, order_, n_traj_, 0, seg_offsets_.data(), T_.data(), coef_.data(), status_.data(), &envelope, box_lo, box_hi,
                                envelope_range_.data(), envelope_norm_.data(), envelope_peak_.data(), envelope_seg_verdict_.data(),
                                verdict.data()) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            verdict.clear();
        }
        return verdict;
    }
    const std::vector<double>& envelopeRange() const { return envelope_range_; }
    const std::vector<double>& envelopeNorm() const { return envelope_norm_; }
    const std::vector<double>& envelopePeak() const { return envelope_peak_; }
    const std::vector<int32_t>& envelopeSegVerdict() const { return envelope_seg_verdict_; }
    // Certified clearance of the stored coefficients at the stored durations against a distance field over WHOLE segments (after solve()
    // or an optimiser; uavqp_clearance_certificate_host).  map: a uavqp::EsdfMap of cpp/esdf_map.h built on context() and updated.
    // Returns the verdict word per trajectory (UAVQP_CLEARANCE_CERTIFIED: at least d_req for ALL t, UAVQP_CLEARANCE_VIOLATED: less at
    // the witness, UAVQP_CLEARANCE_OUTSIDE: a witness point left the map; include/uavqp.h) and fills clearanceBounds() [sum M][2]
    // (lower, upper), clearanceWitness() [sum M], clearancePeak() [n_traj][2], clearanceSegVerdict() [sum M].  A trajectory that did not
    // solve carries zeros.  Empty on failure.
    template <class Map>
    std::vector<int32_t> getClearanceCertificate(const Map& map, const uavqp_clearance_cert_params& params) {
        std::vector<int32_t> verdict;
        if (n_traj_ <= 0 || !ctx_ || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]) ||
            coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || status_.size() != static_cast<size_t>(n_traj_))
            return verdict;
        const size_t tot = static_cast<size_t>(seg_offsets_[n_traj_]);
        verdict.assign(n_traj_, 0);
        clearance_bounds_.assign(2 * tot, 0.0);
        clearance_witness_.assign(tot, 0);
        clearance_peak_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        clearance_seg_verdict_.assign(tot, 0);
        if (uavqp_clearance_certificate_host(ctx_, order_, n_traj_, 0, seg_offsets_.data(), T_.data(), coef_.data(), status_.data(), map.handle(),
                                             &params, clearance_bounds_.data(), clearance_witness_.data(), clearance_peak_.data(),
                                             clearance_seg_verdict_.data(), verdict.data()) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            verdict.clear();
        }
        return verdict;
    }
    const std::vector<double>& clearanceBounds() const { return clearance_bounds_; }
    const std::vector<int32_t>& clearanceWitness() const { return clearance_witness_; }
    const std::vector<double>& clearancePeak() const { return clearance_peak_; }
    const std::vector<int32_t>& clearanceSegVerdict() const { return clearance_seg_verdict_; }
    // optimizeTrajectory for the swarms set with setSwarm (include/uavqp.h uavqp_swarm_optimize_host; the reference's equality rows only:
    // false when a corridor or rows are set): the separation penalty `swarm` between the vehicles of each swarm joins the objective and
    // every trial is accepted or rejected per SWARM.  With params->start_window > 0 the departures of setSwarm are optimised too and the
    // new ones stored (swarmStart()).  Fills the members optimizeTrajectory fills -- objective() [n_groups][2] and acceptedTrials()
    // [n_groups] are per swarm -- and minSep() per trajectory.  params: null = uavqp_default_swarm_opt_params.  All penalties are soft and
    // the result a local minimum: uavqp_time_reallocate_device and uavqp_ellipsoid_check_* afterwards remain the hard tests.
    template <class Map>
    bool optimizeSwarm(const Map& map, const uavqp_limit_params& limits, const uavqp_clearance_params& clearance, const uavqp_swarm_params& swarm,
                       const uavqp_swarm_opt_params* params = nullptr) {
        if (n_traj_ <= 0 || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_])) return false;
        if (!lo_.empty() || rows_k_ > 0) {
            std::cout << "solver solve failed! (optimizeSwarm: corridor and general-rows problems are out of scope)" << std::endl;
            return false;
        }
        if (!start_.empty() && start_.size() != static_cast<size_t>(n_traj_)) return false;
        if (!ensureContext()) return false;
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        uavqp_swarm_opt_params pp;
        if (params) pp = *params; else uavqp_default_swarm_opt_params(&pp);
        if (start_.empty() && pp.start_window > 0.0) start_.assign(n_traj_, 0.0);
        const int n_groups = groups_.empty() ? 1 : static_cast<int>(groups_.size()) - 1;
        coef_.assign(static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_], 0.0);
        status_.assign(n_traj_, 0);
        objective_.assign(static_cast<size_t>(2) * n_groups, 0.0);
        accepted_.assign(n_groups, 0);
        peak_.assign(static_cast<size_t>(2) * n_traj_, 0.0);
        min_dist_.assign(n_traj_, 0.0);
        outside_.assign(n_traj_, 0);
        min_sep_.assign(n_traj_, 0.0);
        const int rc = uavqp_swarm_optimize_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), n_groups,
                                                 groups_.empty() ? nullptr : groups_.data(), start_.empty() ? nullptr : start_.data(),
                                                 map.handle(), &limits, &clearance, &swarm, &pp, coef_.data(), status_.data(), objective_.data(),
                                                 accepted_.data(), peak_.data(), min_dist_.data(), outside_.data(), min_sep_.data());
        if (rc != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        for (int32_t s : status_) if (s != UAVQP_SOLVED) return false;
        return true;
    }
    const std::vector<double>& minSep() const { return min_sep_; }
    const std::vector<double>& swarmStart() const { return start_; }   // (empty: every vehicle departs at 0)
    // Limit penalty + clearance penalty per trajectory of the stored coefficients at the stored durations, in one launch
    // (uavqp_flight_penalty_host).  A trajectory that did not solve carries zero.  Empty on failure.
    template <class Map>
    std::vector<double> getFlightPenalty(const Map& map, const uavqp_limit_params& limits, const uavqp_clearance_params& clearance) {
        std::vector<double> phi;
        if (n_traj_ <= 0 || !ctx_ || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]) ||
            coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || status_.size() != static_cast<size_t>(n_traj_))
            return phi;
        phi.assign(n_traj_, 0.0);
        if (uavqp_flight_penalty_host(ctx_, order_, n_traj_, 0, seg_offsets_.data(), T_.data(), coef_.data(), status_.data(), map.handle(), &limits,
                                      &clearance, phi.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            phi.clear();
        }
        return phi;
    }
    const std::vector<double>& waypoints() const { return wp_; }
    const std::vector<double>& minDist() const { return min_dist_; }
    const std::vector<int32_t>& outsideSamples() const { return outside_; }
    // Gradient of the control cost of the stored coefficients in the waypoints, [sum (M + 1)][3], both ends of every trajectory included
    // (after solve() of an equality-constrained problem; uavqp_cost_waypoint_gradient_host).  Empty on failure.
    std::vector<double> getCostWaypointGradient() {
        std::vector<double> grad;
        if (n_traj_ <= 0 || !ctx_ || !lo_.empty() || rows_k_ > 0 ||
            coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || status_.size() != static_cast<size_t>(n_traj_))
            return grad;
        grad.assign(wp_.size(), 0.0);
        if (uavqp_cost_waypoint_gradient_host(ctx_, order_, n_traj_, 0, seg_offsets_.data(), coef_.data(), status_.data(), grad.data()) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            grad.clear();
        }
        return grad;
    }
    // The context this optimiser solves on (created on first use; nullptr without a device): what a uavqp::EsdfMap is built on.
    uavqp_ctx* context() { return ensureContext() ? ctx_ : nullptr; }
    const std::vector<double>& objective() const { return objective_; }
    const std::vector<int32_t>& acceptedTrials() const { return accepted_; }
    // Control cost c' P c (integral of the squared r-th derivative, three axes) per trajectory of the current waypoints at the current
    // durations: one solve with no iteration and a time weight too small to register in float64 -- the objective then IS the cost.
    // Equality rows only, like optimizeTime; leaves coefficients and durations as they are.  Empty on failure.
    std::vector<double> getCost() {
        std::vector<double> cost;
        if (n_traj_ <= 0 || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]) || !lo_.empty() || rows_k_ > 0 || !ensureContext()) return cost;
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        uavqp_time_opt_params pp;
        uavqp_default_time_opt_params(&pp);
        pp.max_iters = 0;
        pp.time_weight = 1e-300;
        pp.t_min = 1e-300;
        pp.t_max = 1e300;
        std::vector<double> T(T_), coef(static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_], 0.0), obj(static_cast<size_t>(2) * n_traj_, 0.0);
        if (uavqp_time_optimize_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T.data(), bc_.data(), &pp, coef.data(), nullptr,
                                     obj.data(), nullptr) != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return cost;
        }
        cost.resize(n_traj_);
        for (int b = 0; b < n_traj_; ++b) cost[b] = obj[static_cast<size_t>(2) * b + 1];
        return cost;
    }

    // Backward pass of the last solve() (include/uavqp.h uavqp_solve_backward_host; the reference's equality rows only: false when a corridor
    // or rows are set, or before a solve()).  gradCoeff = d loss / d getPolyCoeff(), same layout.  Out: the gradients of the loss through the
    // solve with respect to the durations [sum M], the waypoints [sum (M + 1)][3] and the boundary derivatives [n_traj][2][order-1][3].
    // The explicit dependence of the loss on the durations is the caller's.  A trajectory that did not solve carries zeros.
    bool backward(const std::vector<double>& gradCoeff, std::vector<double>& gradTimes, std::vector<double>& gradWaypoints,
                  std::vector<double>& gradBoundary) {
        if (n_traj_ <= 0 || !ctx_ || !lo_.empty() || rows_k_ > 0) return false;
        if (coef_.size() != static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_] || gradCoeff.size() != coef_.size() ||
            status_.size() != static_cast<size_t>(n_traj_) || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_]))
            return false;
        gradTimes.assign(T_.size(), 0.0);
        gradWaypoints.assign(wp_.size(), 0.0);
        gradBoundary.assign(bc_.size(), 0.0);
        const int rc = uavqp_solve_backward_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), coef_.data(),
                                                 status_.data(), gradCoeff.data(), gradTimes.data(), gradWaypoints.data(), gradBoundary.data());
        if (rc != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        return true;
    }

    // BASELINE config 5 as one call (include/uavqp.h uavqp_corridor_pipeline_host): plain solve -> corridor boxes from the obstacle cloud
    // (SE(3) robot ellipsoid of KinoAstar::isCollisionFree) -> <= max_rounds x (corridor solve + time re-allocation) -> collision check
    // -> repair.  obstacles [n_obs][3].  On return: getPolyCoeff() = the final polynomials, timeAllocation() = the stretched durations,
    // corridorLo() / corridorHi() = the boxes of the final solve, firstHit() = first colliding sample per trajectory (check_samples =
    // free), pipelineResult() = the summary.  true iff the call succeeded and every trajectory is SOLVED (collisions are reported, not
    // turned into failure: a planner decides what to do with a colliding candidate).
    // repair = PipelineRepair::Rows: uavqp_corridor_pipeline_rows_host; repairRowTau() / repairRowDeriv() / repairRowLo() / repairRowHi()
    // then hold the rows of the final solve ([segment][2], [segment][2][3]; deriv -1 = unused), empty after a Boxes call.
    bool solvePipeline(const double* obstacles, int n_obs, const uavqp_pipeline_params* params = nullptr,
                       PipelineRepair repair = PipelineRepair::Boxes) {
        if (n_traj_ <= 0 || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_])) return false;
        if (!ensureContext()) return false;
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        uavqp_pipeline_params pp;
        if (params) pp = *params; else uavqp_default_pipeline_params(&pp);
        coef_.assign(static_cast<size_t>(3) * 2 * order_ * seg_offsets_[n_traj_], 0.0);
        status_.assign(n_traj_, 0);
        // (the pipeline's boxes go to their own members: lo_ / hi_ are what setCorridor() installed and what a later plain solve() keys on -- ADVICE r3)
        pipe_lo_.assign(wp_.size(), 0.0);
        pipe_hi_.assign(wp_.size(), 0.0);
        first_hit_.assign(n_traj_, pp.check_samples);
        pipe_result_ = uavqp_pipeline_result{};
        const size_t n_seg = static_cast<size_t>(seg_offsets_[n_traj_]);
        const bool rows = repair == PipelineRepair::Rows;
        repair_tau_.assign(rows ? 2 * n_seg : 0, 0.0);
        repair_deriv_.assign(rows ? 2 * n_seg : 0, -1);
        repair_lo_.assign(rows ? 6 * n_seg : 0, 0.0);
        repair_hi_.assign(rows ? 6 * n_seg : 0, 0.0);
        const int rc = rows ? uavqp_corridor_pipeline_rows_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), obstacles,
                                                                n_obs, &pp, coef_.data(), status_.data(), pipe_lo_.data(), pipe_hi_.data(), first_hit_.data(),
                                                                repair_tau_.data(), repair_deriv_.data(), repair_lo_.data(), repair_hi_.data(), &pipe_result_)
                            : uavqp_corridor_pipeline_host(ctx_, order_, n_traj_, 0, 0, seg_offsets_.data(), wp_.data(), T_.data(), bc_.data(), obstacles, n_obs,
                                                           &pp, coef_.data(), status_.data(), pipe_lo_.data(), pipe_hi_.data(), first_hit_.data(), &pipe_result_);
        if (rc != UAVQP_OK) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        return pipe_result_.unsolved == 0;
    }
    const std::vector<double>& timeAllocation() const { return T_; }
    const std::vector<double>& corridorLo() const { return pipe_lo_; }   // boxes of the last solvePipeline() (setCorridor()'s own are untouched)
    const std::vector<double>& corridorHi() const { return pipe_hi_; }
    const std::vector<int32_t>& firstHit() const { return first_hit_; }
    const uavqp_pipeline_result& pipelineResult() const { return pipe_result_; }
    int repairRows() const { return pipe_result_.repair_rows; }                  // rows placed and kept by the last Rows repair
    const std::vector<double>& repairRowTau() const { return repair_tau_; }
    const std::vector<int32_t>& repairRowDeriv() const { return repair_deriv_; }
    const std::vector<double>& repairRowLo() const { return repair_lo_; }
    const std::vector<double>& repairRowHi() const { return repair_hi_; }

    // ---- multi-GPU: one process (or thread) per GPU, every rank holds the whole batch description, solves its contiguous shard
    // (balanced by segment count) on its device and ends with ALL coefficients: uavqp_shard_bounds_ragged, uavqp_comm_create,
    // uavqp_solve_*_batch_device on views, uavqp_allgather_coeffs / _status (RCCL over xGMI).  Rank 0 draws the id and ships it to
    // the others with whatever the program has (MPI_Bcast, a socket, a file).
    static bool uniqueId(unsigned char* id_out /* UAVQP_UNIQUE_ID_BYTES */) { return uavqp_comm_unique_id(id_out) == UAVQP_OK; }
    bool initDistributed(int rank, int world, const unsigned char* unique_id) {
        if (!ensureContext()) return false;
        rank_ = rank;
        world_ = world;
        if (uavqp_comm_create(ctx_, rank, world, unique_id) != UAVQP_OK) {
            std::cout << "solver init failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        return true;
    }
#ifdef UAVQP_TRAJ_OPTIMIZER_HAS_HIP
    bool solveSharded() {
        if (n_traj_ <= 0 || world_ < 1 || !ctx_ || T_.size() != static_cast<size_t>(seg_offsets_[n_traj_])) return false;
        if (!rowsMatchBatch() || !corridorMatchesBatch()) {
            std::cout << "solver solve failed! (rows or corridor arrays do not match the current batch)" << std::endl;
            return false;
        }
        if (bc_.empty()) bc_.assign(static_cast<size_t>(n_traj_) * 2 * (order_ - 1) * 3, 0.0);
        std::vector<int32_t> bounds(world_ + 1);
        if (uavqp_shard_bounds_ragged(seg_offsets_.data(), n_traj_, world_, bounds.data()) != UAVQP_OK) return false;
        const int b0 = bounds[rank_], b1 = bounds[rank_ + 1], nl = b1 - b0;
        const int32_t s0 = seg_offsets_[b0], s1 = seg_offsets_[b1];
        const size_t nc = static_cast<size_t>(3) * 2 * order_, tot = static_cast<size_t>(seg_offsets_[n_traj_]);
        std::vector<int32_t> so_l(nl + 1);
        int mmax = 1;
        for (int b = 0; b <= nl; ++b) so_l[b] = seg_offsets_[b0 + b] - s0;
        for (int b = 0; b < nl; ++b) mmax = std::max(mmax, so_l[b + 1] - so_l[b]);
        std::vector<int64_t> c_counts(world_), t_counts(world_);
        size_t c_off = 0;
        for (int g = 0; g < world_; ++g) {
            c_counts[g] = static_cast<int64_t>(nc) * (seg_offsets_[bounds[g + 1]] - seg_offsets_[bounds[g]]);
            t_counts[g] = bounds[g + 1] - bounds[g];
            if (g < rank_) c_off += static_cast<size_t>(c_counts[g]);
        }
        const size_t n_wp = static_cast<size_t>(3) * ((s1 - s0) + nl), n_t = static_cast<size_t>(s1 - s0), n_bc = static_cast<size_t>(nl) * 2 * (order_ - 1) * 3;
        int32_t *d_so = nullptr, *d_st = nullptr, *d_rd = nullptr;
        double *d_wp = nullptr, *d_T = nullptr, *d_bc = nullptr, *d_lo = nullptr, *d_hi = nullptr, *d_coef = nullptr, *d_rt = nullptr, *d_rl = nullptr, *d_rh = nullptr;
        bool ok = hipSetDevice(device_) == hipSuccess;
        auto up = [&](void** d, const void* h, size_t bytes) {
            ok = ok && hipMalloc(d, bytes ? bytes : 8) == hipSuccess && (bytes == 0 || hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) == hipSuccess);
        };
        up(reinterpret_cast<void**>(&d_so), so_l.data(), sizeof(int32_t) * (nl + 1));
        up(reinterpret_cast<void**>(&d_wp), wp_.data() + static_cast<size_t>(3) * (s0 + b0), sizeof(double) * n_wp);
        up(reinterpret_cast<void**>(&d_T), T_.data() + s0, sizeof(double) * n_t);
        up(reinterpret_cast<void**>(&d_bc), bc_.data() + static_cast<size_t>(b0) * 2 * (order_ - 1) * 3, sizeof(double) * n_bc);
        if (!lo_.empty()) {
            up(reinterpret_cast<void**>(&d_lo), lo_.data() + static_cast<size_t>(3) * (s0 + b0), sizeof(double) * n_wp);
            up(reinterpret_cast<void**>(&d_hi), hi_.data() + static_cast<size_t>(3) * (s0 + b0), sizeof(double) * n_wp);
        }
        if (rows_k_ > 0) {   // the shard's general inequality rows (per segment, rows_k_ slots)
            const size_t k = static_cast<size_t>(rows_k_);
            up(reinterpret_cast<void**>(&d_rt), row_tau_.data() + k * s0, sizeof(double) * k * n_t);
            up(reinterpret_cast<void**>(&d_rd), row_deriv_.data() + k * s0, sizeof(int32_t) * k * n_t);
            up(reinterpret_cast<void**>(&d_rl), row_lo_.data() + 3 * k * s0, sizeof(double) * 3 * k * n_t);
            up(reinterpret_cast<void**>(&d_rh), row_hi_.data() + 3 * k * s0, sizeof(double) * 3 * k * n_t);
        }
        ok = ok && hipMalloc(reinterpret_cast<void**>(&d_coef), sizeof(double) * nc * tot) == hipSuccess &&
             hipMalloc(reinterpret_cast<void**>(&d_st), sizeof(int32_t) * n_traj_) == hipSuccess;
        // the device kernels leave a trajectory they flag UAVQP_INVALID_INPUT untouched: zeros, as the host entry points give
        ok = ok && hipMemset(d_coef, 0, sizeof(double) * nc * tot) == hipSuccess && hipMemset(d_st, 0, sizeof(int32_t) * n_traj_) == hipSuccess;
        int rc = ok ? UAVQP_OK : UAVQP_ERR_ALLOC;
        if (ok && nl > 0) {   // this rank's shard, written straight into its slice of the full buffers
            if (rows_k_ > 0)
                rc = uavqp_solve_rows_batch_device(ctx_, order_, nl, 0, mmax, d_so, d_wp, d_T, d_bc, d_lo, d_hi, rows_k_, d_rt, d_rd, d_rl, d_rh,
                                                   d_coef + c_off, d_st + b0, nullptr, nullptr);
            else if (lo_.empty())
                rc = uavqp_solve_batch_device(ctx_, order_, nl, 0, mmax, d_so, d_wp, d_T, d_bc, d_coef + c_off, d_st + b0);
            else
                rc = uavqp_solve_corridor_batch_device(ctx_, order_, nl, 0, mmax, d_so, d_wp, d_T, d_bc, d_lo, d_hi, d_coef + c_off, d_st + b0, nullptr);
        }
        if (rc == UAVQP_OK) rc = uavqp_allgather_coeffs(ctx_, d_coef + c_off, c_counts.data(), d_coef);
        if (rc == UAVQP_OK) rc = uavqp_allgather_status(ctx_, d_st + b0, t_counts.data(), d_st);
        if (rc == UAVQP_OK) rc = uavqp_synchronize(ctx_);
        coef_.assign(nc * tot, 0.0);
        status_.assign(n_traj_, 0);
        if (rc == UAVQP_OK) {
            ok = hipMemcpy(coef_.data(), d_coef, sizeof(double) * nc * tot, hipMemcpyDeviceToHost) == hipSuccess &&
                 hipMemcpy(status_.data(), d_st, sizeof(int32_t) * n_traj_, hipMemcpyDeviceToHost) == hipSuccess;
        }
        for (void* p : {static_cast<void*>(d_so), static_cast<void*>(d_st), static_cast<void*>(d_wp), static_cast<void*>(d_T), static_cast<void*>(d_bc),
                        static_cast<void*>(d_lo), static_cast<void*>(d_hi), static_cast<void*>(d_coef), static_cast<void*>(d_rt), static_cast<void*>(d_rd),
                        static_cast<void*>(d_rl), static_cast<void*>(d_rh)})
            if (p) (void)hipFree(p);
        if (rc != UAVQP_OK || !ok) {
            std::cout << "solver solve failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        for (int32_t s : status_) if (s != UAVQP_SOLVED) return false;
        return true;
    }
#endif

  private:
    bool rowsMatchBatch() const {
        if (rows_k_ <= 0) return true;
        const size_t n = T_.size() * static_cast<size_t>(rows_k_);
        return row_tau_.size() == n && row_deriv_.size() == n && row_lo_.size() == 3 * n && row_hi_.size() == 3 * n;
    }
    bool corridorMatchesBatch() const { return lo_.empty() || (lo_.size() == wp_.size() && hi_.size() == wp_.size()); }
    bool ensureContext() {
        if (ctx_) return true;
        if (uavqp_create(&ctx_, device_) != UAVQP_OK) {
            std::cout << "solver init failed! (" << uavqp_last_error() << ")" << std::endl;
            ctx_ = nullptr;
            return false;
        }
        if (have_settings_ && uavqp_set_settings(ctx_, &settings_) != UAVQP_OK) {
            std::cout << "solver init failed! (" << uavqp_last_error() << ")" << std::endl;
            return false;
        }
        return true;
    }

    int order_, device_, n_traj_ = 0;
    int rank_ = 0, world_ = 1;
    bool have_settings_ = false;
    uavqp_settings settings_{};
    uavqp_ctx* ctx_ = nullptr;
    std::vector<int32_t> seg_offsets_, status_;
    std::vector<double> wp_, T_, bc_, coef_, lo_, hi_, pipe_lo_, pipe_hi_, row_tau_, row_lo_, row_hi_;
    std::vector<int32_t> row_deriv_, first_hit_, repair_deriv_;
    std::vector<double> repair_tau_, repair_lo_, repair_hi_;
    std::vector<double> objective_, peak_, min_dist_, min_sep_, attitude_peak_, envelope_range_, envelope_norm_, envelope_peak_;
    std::vector<int32_t> envelope_seg_verdict_, clearance_witness_, clearance_seg_verdict_;
    std::vector<double> clearance_bounds_, clearance_peak_;
    std::vector<int32_t> outside_;
    std::vector<int32_t> accepted_;
    std::vector<double> separation_lower_, separation_upper_;
    std::vector<int32_t> separation_where_, separation_group_verdict_;
    // setMovingObstacles: copies of the arrays of a uavqp_moving_obstacles (empty = that pointer is NULL)
    struct MovingStore {
        bool set = false;
        int32_t n_obs = 0, uniform_segments = 0, n_sets = 0;
        std::vector<int32_t> seg_offsets, set_offsets, traj_set;
        std::vector<double> times, coeff, start, radius, traj_start;
        uavqp_moving_obstacles view() const {
            uavqp_moving_obstacles o;
            o.struct_size = static_cast<int32_t>(sizeof(uavqp_moving_obstacles));
            o.n_obs = n_obs; o.uniform_segments = uniform_segments; o.n_sets = n_sets;
            o.seg_offsets = seg_offsets.empty() ? nullptr : seg_offsets.data();
            o.times = times.empty() ? nullptr : times.data();
            o.coeff = coeff.empty() ? nullptr : coeff.data();
            o.start = start.empty() ? nullptr : start.data();
            o.radius = radius.empty() ? nullptr : radius.data();
            o.set_offsets = set_offsets.empty() ? nullptr : set_offsets.data();
            o.traj_set = traj_set.empty() ? nullptr : traj_set.data();
            o.traj_start = traj_start.empty() ? nullptr : traj_start.data();
            return o;
        }
    };
    MovingStore moving_;
    std::vector<double> min_gap_;
    std::vector<int32_t> nearest_;
    std::vector<double> moving_gap_, moving_peak_;
    std::vector<int32_t> moving_where_, moving_seg_verdict_;
    std::vector<int32_t> groups_;   // setSwarm: empty = the whole batch is one swarm
    std::vector<double> start_;     // setSwarm: empty = every vehicle departs at 0
    int rows_k_ = 0;
    uavqp_pipeline_result pipe_result_{};
};

}  // namespace traj_optimization
#endif
