// uavqp_spacetime_lbfgs.h -- host side of uavqp_spacetime_lbfgs_device / _host, uavqp_attitude_optimize_device / _host and
// uavqp_moving_optimize_device / _host (include/uavqp.h):
// included by uavqp.hip behind uavqp_spacetime.h, whose parameter checks, penalty launch and sequencing it shares, uavqp_attitude.h and
// uavqp_moving.h.  Kernel: qp_spacetime_lbfgs.h (translation unit k_spacetime_lbfgs.hip).
//
// The launch sequence is that of uavqp_spacetime_optimize_device with the other step kernel: NO data-dependent control flow on the host, the
// number of launches is fixed by max_iters, every decision (accept / reject, which pairs are kept, quasi-Newton or gradient direction, a
// reset of the memory) is taken per trajectory on the device, and nothing is read back:
//     anchor copy -> clamp -> solve(waypoints, times) -> flight penalty -> backward -> step<INIT>
//       -> max_iters x { solve(trial waypoints, trial durations) -> flight penalty -> backward -> step<ITER> }
//       -> solve(waypoints, times) -> flight penalty (peak / min_dist / outside only)
// Four launches per iteration; with the attitude penalty (uavqp_attitude_optimize_device) one more after every flight penalty of the loop,
// with the moving-obstacle penalty (uavqp_moving_optimize_device) one more behind that: six at the most.
#pragma once

extern "C" void uavqp_default_spacetime_lbfgs_params(uavqp_spacetime_lbfgs_params* p) {
    if (!p) return;
    uavqp_spacetime_params s;
    uavqp_default_spacetime_params(&s);
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_spacetime_lbfgs_params);
    p->max_iters = s.max_iters;    // the two entries compare at equal cost
    p->memory = 8;                 // CPU transcription against L-BFGS-B on the test scenes: DESIGN.md section 5.21
    p->max_backtracks = 6;
    p->smooth_weight = s.smooth_weight;
    p->time_weight = s.time_weight;
    p->t_min = s.t_min;
    p->t_max = s.t_max;
    p->max_move = s.max_move;
    p->initial_step_move = s.initial_step_move;
    p->initial_step_log = s.initial_step_log;
    p->armijo_c = s.armijo_c;
    p->shrink = s.shrink;
    p->grow = s.grow;
    p->curvature_eps = 1e-10;
}

static bool spacetime_lbfgs_params_valid(const uavqp_spacetime_lbfgs_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_spacetime_lbfgs_params)) return false;
    const uavqp_spacetime_params s = spacetime_part_of(*p);
    if (!spacetime_params_valid(&s)) return false;
    if (p->memory < 1 || p->memory > UAVQP_LBFGS_MAX_MEMORY) return false;
    if (p->max_backtracks < 1 || p->max_backtracks > 64) return false;
    if (!(p->curvature_eps >= 0.0 && p->curvature_eps < 1.0)) return false;
    return true;
}

// The sequence above for both entries.  attitude null (uavqp_spacetime_lbfgs_device): exactly those launches.  attitude with a positive
// weight (uavqp_attitude_optimize_device): the accumulating attitude penalty (qp_attitude.h) is enqueued between the flight penalty and the
// backward pass, so the step kernel reads the summed phi and the summed partial gradients -- five launches per iteration.  obstacles and
// moving (uavqp_moving_optimize_device; both or neither) with a positive weight and an obstacle to avoid: the accumulating moving-obstacle
// penalty (qp_moving.h) follows the attitude launch in the same way, and its min_gap / nearest are taken at what is handed back.
static int spacetime_lbfgs_run(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                               const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc, const uavqp_esdf* esdf,
                               const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                               const uavqp_spacetime_lbfgs_params* params, double* d_coeff_out, int32_t* d_status_out, double* d_objective_out,
                               int32_t* d_accepted_out, double* d_peak_out, double* d_min_dist_out, int32_t* d_outside_out,
                               const uavqp_attitude_params* attitude, double* d_attitude_peak_out,
                               const uavqp_moving_obstacles* obstacles = nullptr, const uavqp_moving_params* moving = nullptr,
                               double* d_min_gap_out = nullptr, int32_t* d_nearest_out = nullptr) {
    bool run;
    int rc = descent_args_check(ctx, r, n_traj, 1, uniform_segments, max_segments, total_segments, d_seg_offsets,
                                d_waypoints && d_times && d_bc && d_coeff_out && d_objective_out, true, [&] {
                                    return spacetime_lbfgs_params_valid(params) && flight_params_valid(ctx, esdf, limits, clearance) &&
                                           (!attitude || attitude_params_valid(attitude)) &&
                                           (!moving || (moving_params_valid(moving) && moving_obstacles_valid(obstacles)));
                                }, &run);
    if (!run) return rc;
    const bool with_attitude = attitude && attitude_any_weight(*attitude);
    const bool with_moving = moving && moving->weight > 0.0 && !moving_nothing_to_avoid(*obstacles);
    const uavqp_spacetime_lbfgs_params P = *params;
    const size_t n = (size_t)n_traj, tot = (size_t)total_segments;
    const size_t slots = P.max_iters > 0 ? (size_t)P.memory + 1 : 0;   // (no trial: no pair is ever written)

    JointRun j{ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_times, d_bc, esdf, limits, clearance,
               d_coeff_out, d_status_out};
    Carve& c = j.c;
    j.k.declare(c, r, n, tot);
    const size_t wp_bytes = j.k.wp_bytes, t_bytes = j.k.t_bytes;
    const int i_fb = c.add(sizeof(double) * n), i_al = c.add(sizeof(double) * n), i_nd = c.add(sizeof(double) * n), i_sg = c.add(sizeof(double) * 2 * n);
    // the history (memory + 1 slots of s and y in the layout of the waypoints plus the durations), the direction, the free set, the state
    const int i_sp = c.add(slots * wp_bytes), i_yp = c.add(slots * wp_bytes), i_su = c.add(slots * t_bytes), i_yu = c.add(slots * t_bytes);
    const int i_dp = c.add(wp_bytes), i_du = c.add(t_bytes), i_fp = c.add(wp_bytes), i_fu = c.add(t_bytes);
    const int i_state = c.add(sizeof(int32_t) * 4 * n);
    rc = carve_on(ctx->stream, ctx->topt, c);
    if (rc != UAVQP_OK) return rc;

    uavqp::SpacetimeLbfgsArgs q;
    uavqp::SpacetimeArgs& a = q.g;
    j.fill(a, P, d_objective_out, d_accepted_out);
    a.fbest = c.at<double>(i_fb); a.alpha = c.at<double>(i_al); a.need = c.at<double>(i_nd); a.sigma = c.at<double>(i_sg);
    q.hist_sp = c.at<double>(i_sp); q.hist_yp = c.at<double>(i_yp); q.hist_su = c.at<double>(i_su); q.hist_yu = c.at<double>(i_yu);
    q.dir_p = c.at<double>(i_dp); q.dir_u = c.at<double>(i_du); q.free_p = c.at<double>(i_fp); q.free_u = c.at<double>(i_fu);
    q.state = c.at<int32_t>(i_state);
    q.wp_len = 3 * (tot + n); q.t_len = tot;
    q.memory = P.memory; q.max_backtracks = P.max_backtracks; q.curvature_eps = P.curvature_eps;
    const int grid = topt_grid(ctx, n_traj);
    // the accumulating attitude penalty, then the accumulating moving-obstacle penalty, between the flight penalty and the backward pass
    auto attitude_penalty = [&](const DescentPoint& p) -> int {
        int e = UAVQP_OK;
        if (with_attitude)
            e = attitude_penalty_enqueue(ctx, j.solved_at(p), *attitude, j.at<double>(j.k.ph), j.at<double>(j.k.g), j.at<double>(j.k.ex), nullptr,
                                         true);
        if (e == UAVQP_OK && with_moving)
            e = moving_penalty_enqueue(ctx, j.solved_at(p), *obstacles, *moving, j.at<double>(j.k.ph), j.at<double>(j.k.g), j.at<double>(j.k.ex),
                                       nullptr, nullptr, nullptr, true);
        return e;
    };
    rc = j.anchor_copies(P.max_iters);
    if (rc == UAVQP_OK) rc = time_clamp_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, P.t_min, P.t_max);
    if (rc == UAVQP_OK)
        rc = j.descend(a, P.max_iters, attitude_penalty, [&](auto R, auto INIT) {
            constexpr auto kernel = uavqp::spacetime_lbfgs_step_kernel<decltype(R)::value, decltype(INIT)::value>;
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, ctx->stream, q);
        });
    if (rc == UAVQP_OK) rc = j.flight_diagnostics(d_peak_out, d_min_dist_out, d_outside_out);
    if (rc == UAVQP_OK && attitude && d_attitude_peak_out)
        rc = attitude_penalty_enqueue(ctx, j.solved_final(), *attitude, nullptr, nullptr, nullptr, d_attitude_peak_out);
    if (rc == UAVQP_OK && moving && (d_min_gap_out || d_nearest_out))
        rc = moving_penalty_enqueue(ctx, j.solved_final(), *obstacles, *moving, nullptr, nullptr, nullptr, nullptr, d_min_gap_out, d_nearest_out);
    return rc;
}

extern "C" int uavqp_spacetime_lbfgs_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                            const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc,
                                            const uavqp_esdf* esdf, const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                            const uavqp_spacetime_lbfgs_params* params, double* d_coeff_out, int32_t* d_status_out,
                                            double* d_objective_out, int32_t* d_accepted_out, double* d_peak_out, double* d_min_dist_out,
                                            int32_t* d_outside_out) {
    return spacetime_lbfgs_run(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_times, d_bc, esdf,
                               limits, clearance, params, d_coeff_out, d_status_out, d_objective_out, d_accepted_out, d_peak_out, d_min_dist_out,
                               d_outside_out, nullptr, nullptr);
}

extern "C" int uavqp_attitude_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                              const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc,
                                              const uavqp_esdf* esdf, const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                              const uavqp_attitude_params* attitude, const uavqp_spacetime_lbfgs_params* params,
                                              double* d_coeff_out, int32_t* d_status_out, double* d_objective_out, int32_t* d_accepted_out,
                                              double* d_peak_out, double* d_min_dist_out, int32_t* d_outside_out, double* d_attitude_peak_out) {
    if (!attitude_params_valid(attitude)) return UAVQP_ERR_INVALID_ARG;
    return spacetime_lbfgs_run(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_times, d_bc, esdf,
                               limits, clearance, params, d_coeff_out, d_status_out, d_objective_out, d_accepted_out, d_peak_out, d_min_dist_out,
                               d_outside_out, attitude, d_attitude_peak_out);
}

// both _host entries: the staging of uavqp_spacetime_optimize_host (descent_run_host) around spacetime_lbfgs_run
static int spacetime_lbfgs_run_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                    double* waypoints, double* times, const double* bc, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                                    const uavqp_clearance_params* clearance, const uavqp_spacetime_lbfgs_params* params, double* coeff_out,
                                    int32_t* status_out, double* objective_out, int32_t* accepted_out, double* peak_out, double* min_dist_out,
                                    int32_t* outside_out, const uavqp_attitude_params* attitude, double* attitude_peak_out, const char* what) {
    return descent_run_host(
        ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, waypoints, times, times, bc,
        [&] {
            return spacetime_lbfgs_params_valid(params) && flight_params_valid(ctx, esdf, limits, clearance) &&
                   (!attitude || attitude_params_valid(attitude));
        },
        coeff_out, status_out, objective_out, accepted_out, peak_out, min_dist_out, outside_out, attitude ? attitude_peak_out : nullptr, 4, what,
        [&](const DescentStaged& d) {
            return spacetime_lbfgs_run(ctx, r, n_traj, uniform_segments, d.Mmax, d.total_segments, d.seg_offsets, d.waypoints, d.times, d.bc, esdf,
                                       limits, clearance, params, d.coeff, d.status, d.objective, d.accepted, d.peak, d.min_dist, d.outside,
                                       attitude, d.extra);
        });
}

extern "C" int uavqp_spacetime_lbfgs_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                          double* waypoints, double* times, const double* bc, const uavqp_esdf* esdf,
                                          const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                          const uavqp_spacetime_lbfgs_params* params, double* coeff_out, int32_t* status_out, double* objective_out,
                                          int32_t* accepted_out, double* peak_out, double* min_dist_out, int32_t* outside_out) {
    return spacetime_lbfgs_run_host(ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, times, bc, esdf, limits, clearance,
                                    params, coeff_out, status_out, objective_out, accepted_out, peak_out, min_dist_out, outside_out, nullptr,
                                    nullptr, "uavqp_spacetime_lbfgs_host");
}

extern "C" int uavqp_attitude_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                            double* waypoints, double* times, const double* bc, const uavqp_esdf* esdf,
                                            const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                            const uavqp_attitude_params* attitude, const uavqp_spacetime_lbfgs_params* params, double* coeff_out,
                                            int32_t* status_out, double* objective_out, int32_t* accepted_out, double* peak_out,
                                            double* min_dist_out, int32_t* outside_out, double* attitude_peak_out) {
    if (!attitude_params_valid(attitude)) return UAVQP_ERR_INVALID_ARG;
    return spacetime_lbfgs_run_host(ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, times, bc, esdf, limits, clearance,
                                    params, coeff_out, status_out, objective_out, accepted_out, peak_out, min_dist_out, outside_out, attitude,
                                    attitude_peak_out, "uavqp_attitude_optimize_host");
}

extern "C" int uavqp_moving_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                            const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc,
                                            const uavqp_esdf* esdf, const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                            const uavqp_attitude_params* attitude, const uavqp_moving_obstacles* obstacles,
                                            const uavqp_moving_params* moving, const uavqp_spacetime_lbfgs_params* params, double* d_coeff_out,
                                            int32_t* d_status_out, double* d_objective_out, int32_t* d_accepted_out, double* d_peak_out,
                                            double* d_min_dist_out, int32_t* d_outside_out, double* d_attitude_peak_out, double* d_min_gap_out,
                                            int32_t* d_nearest_out) {
    if (!moving_params_valid(moving) || !moving_obstacles_valid(obstacles)) return UAVQP_ERR_INVALID_ARG;
    return spacetime_lbfgs_run(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_times, d_bc, esdf,
                               limits, clearance, params, d_coeff_out, d_status_out, d_objective_out, d_accepted_out, d_peak_out, d_min_dist_out,
                               d_outside_out, attitude, d_attitude_peak_out, obstacles, moving, d_min_gap_out, d_nearest_out);
}

// the staging of spacetime_lbfgs_run_host with the obstacle arrays and the two further outputs declared on the same Stage
extern "C" int uavqp_moving_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                          double* waypoints, double* times, const double* bc, const uavqp_esdf* esdf,
                                          const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                          const uavqp_attitude_params* attitude, const uavqp_moving_obstacles* obstacles,
                                          const uavqp_moving_params* moving, const uavqp_spacetime_lbfgs_params* params, double* coeff_out,
                                          int32_t* status_out, double* objective_out, int32_t* accepted_out, double* peak_out,
                                          double* min_dist_out, int32_t* outside_out, double* attitude_peak_out, double* min_gap_out,
                                          int32_t* nearest_out) {
    if (!moving_params_valid(moving) || !moving_obstacles_valid(obstacles)) return UAVQP_ERR_INVALID_ARG;
    if (n_traj < 0) return UAVQP_ERR_INVALID_ARG;
    BatchShape osh;
    const int rc = moving_host_check(*obstacles, n_traj, &osh);
    if (rc != UAVQP_OK) return rc;
    MovingStage ms;
    int i_mg = -1, i_nr = -1;
    return descent_run_host(
        ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, waypoints, times, times, bc,
        [&] {
            return spacetime_lbfgs_params_valid(params) && flight_params_valid(ctx, esdf, limits, clearance) &&
                   (!attitude || attitude_params_valid(attitude));
        },
        coeff_out, status_out, objective_out, accepted_out, peak_out, min_dist_out, outside_out, attitude ? attitude_peak_out : nullptr, 4,
        "uavqp_moving_optimize_host",
        [&](const DescentStaged& d, const Stage& st) {
            const uavqp_moving_obstacles dev = ms.device(st, *obstacles);
            return spacetime_lbfgs_run(ctx, r, n_traj, uniform_segments, d.Mmax, d.total_segments, d.seg_offsets, d.waypoints, d.times, d.bc, esdf,
                                       limits, clearance, params, d.coeff, d.status, d.objective, d.accepted, d.peak, d.min_dist, d.outside,
                                       attitude, d.extra, &dev, moving, st.at<double>(i_mg), st.at<int32_t>(i_nr));
        },
        [&](Stage& st) {
            ms.declare(st, *obstacles, r, n_traj, osh);
            i_mg = min_gap_out ? st.out(min_gap_out, sizeof(double) * (size_t)n_traj) : -1;
            i_nr = nearest_out ? st.out(nearest_out, sizeof(int32_t) * (size_t)n_traj) : -1;
        });
}
