// uavqp_spacetime_lbfgs.h -- host side of uavqp_spacetime_lbfgs_device / _host and uavqp_attitude_optimize_device / _host (include/uavqp.h):
// included by uavqp.hip behind uavqp_spacetime.h, whose parameter checks, penalty launch and sequencing it shares, and uavqp_attitude.h.  Kernel: qp_spacetime_lbfgs.h (translation unit
// k_spacetime_lbfgs.hip).
//
// The launch sequence is that of uavqp_spacetime_optimize_device with the other step kernel: NO data-dependent control flow on the host, the
// number of launches is fixed by max_iters, every decision (accept / reject, which pairs are kept, quasi-Newton or gradient direction, a
// reset of the memory) is taken per trajectory on the device, and nothing is read back:
//     anchor copy -> clamp -> solve(waypoints, times) -> flight penalty -> backward -> step<INIT>
//       -> max_iters x { solve(trial waypoints, trial durations) -> flight penalty -> backward -> step<ITER> }
//       -> solve(waypoints, times) -> flight penalty (peak / min_dist / outside only)
// Four launches per iteration; with the attitude penalty (uavqp_attitude_optimize_device) one more after every flight penalty of the loop.
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

// the shared fields as the parameters of the projected-gradient entry (whose validity rule they follow)
static uavqp_spacetime_params spacetime_lbfgs_shared(const uavqp_spacetime_lbfgs_params* p) {
    uavqp_spacetime_params s;
    std::memset(&s, 0, sizeof(s));
    s.struct_size = (int32_t)sizeof(s);
    s.max_iters = p->max_iters;
    s.smooth_weight = p->smooth_weight; s.time_weight = p->time_weight; s.t_min = p->t_min; s.t_max = p->t_max; s.max_move = p->max_move;
    s.initial_step_move = p->initial_step_move; s.initial_step_log = p->initial_step_log; s.armijo_c = p->armijo_c; s.shrink = p->shrink;
    s.grow = p->grow;
    return s;
}

static bool spacetime_lbfgs_params_valid(const uavqp_spacetime_lbfgs_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_spacetime_lbfgs_params)) return false;
    const uavqp_spacetime_params s = spacetime_lbfgs_shared(p);
    if (!spacetime_params_valid(&s)) return false;
    if (p->memory < 1 || p->memory > UAVQP_LBFGS_MAX_MEMORY) return false;
    if (p->max_backtracks < 1 || p->max_backtracks > 64) return false;
    if (!(p->curvature_eps >= 0.0 && p->curvature_eps < 1.0)) return false;
    return true;
}

// The sequence above for both entries.  attitude null (uavqp_spacetime_lbfgs_device): exactly those launches.  attitude with a positive
// weight (uavqp_attitude_optimize_device): the accumulating attitude penalty (qp_attitude.h) is enqueued between the flight penalty and the
// backward pass, so the step kernel reads the summed phi and the summed partial gradients -- five launches per iteration.
static int spacetime_lbfgs_run(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                               const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc, const uavqp_esdf* esdf,
                               const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                               const uavqp_spacetime_lbfgs_params* params, double* d_coeff_out, int32_t* d_status_out, double* d_objective_out,
                               int32_t* d_accepted_out, double* d_peak_out, double* d_min_dist_out, int32_t* d_outside_out,
                               const uavqp_attitude_params* attitude, double* d_attitude_peak_out) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || total_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (!spacetime_lbfgs_params_valid(params) || !limit_params_valid(limits)) return UAVQP_ERR_INVALID_ARG;
    if (!esdf_usable(ctx, esdf) || !esdf->updated || !clearance_params_valid(clearance)) return UAVQP_ERR_INVALID_ARG;
    if (attitude && !attitude_params_valid(attitude)) return UAVQP_ERR_INVALID_ARG;
    const bool with_attitude = attitude && attitude_any_weight(*attitude);
    if (n_traj == 0) return UAVQP_OK;
    if (!d_waypoints || !d_times || !d_bc || !d_coeff_out || !d_objective_out) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && (!d_seg_offsets || max_segments < 1)) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments > 0 && (long long)total_segments != (long long)uniform_segments * n_traj) return UAVQP_ERR_INVALID_ARG;
    if ((long long)total_segments > 0x7fffffffLL - n_traj) return UAVQP_ERR_INVALID_ARG;   // (the waypoint rows are counted in ints)
    UAVQP_HIP(hipSetDevice(ctx->device));
    const uavqp_spacetime_lbfgs_params P = *params;
    const size_t n = (size_t)n_traj, tot = (size_t)total_segments, wp_bytes = sizeof(double) * 3 * (tot + n), t_bytes = sizeof(double) * tot;
    const size_t slots = P.max_iters > 0 ? (size_t)P.memory + 1 : 0;   // (no trial: no pair is ever written)

    Carve c;
    const int i_wt = c.add(wp_bytes), i_an = c.add(wp_bytes), i_gp = c.add(wp_bytes), i_thp = c.add(wp_bytes);
    const int i_t0 = c.add(t_bytes), i_t1 = c.add(t_bytes), i_gt = c.add(t_bytes), i_tht = c.add(t_bytes), i_ex = c.add(t_bytes);
    const int i_g = c.add(sizeof(double) * 3 * 2 * r * tot);
    const int i_ph = c.add(sizeof(double) * n), i_fb = c.add(sizeof(double) * n), i_al = c.add(sizeof(double) * n), i_nd = c.add(sizeof(double) * n);
    const int i_sg = c.add(sizeof(double) * 2 * n), i_ac = c.add(sizeof(int32_t) * n), i_st = c.add(sizeof(int32_t) * n);
    // the history (memory + 1 slots of s and y in the layout of the waypoints plus the durations), the direction, the free set, the state
    const int i_sp = c.add(slots * wp_bytes), i_yp = c.add(slots * wp_bytes), i_su = c.add(slots * t_bytes), i_yu = c.add(slots * t_bytes);
    const int i_dp = c.add(wp_bytes), i_du = c.add(t_bytes), i_fp = c.add(wp_bytes), i_fu = c.add(t_bytes);
    const int i_state = c.add(sizeof(int32_t) * 4 * n);
    int rc = carve_on(ctx->stream, ctx->topt, c);
    if (rc != UAVQP_OK) return rc;
    int32_t* d_st_loop = c.at<int32_t>(i_st);
    int32_t* d_st_final = d_status_out ? d_status_out : d_st_loop;
    double* d_trial_t[2] = {c.at<double>(i_t0), c.at<double>(i_t1)};

    uavqp::SpacetimeLbfgsArgs q;
    uavqp::SpacetimeArgs& a = q.g;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.seg_offsets = d_seg_offsets;
    a.waypoints = d_waypoints; a.wp_trial = c.at<double>(i_wt); a.anchor = c.at<double>(i_an); a.gp_best = c.at<double>(i_gp);
    a.times = d_times; a.t_eval = d_times; a.t_next = d_trial_t[0]; a.gt_best = c.at<double>(i_gt);
    a.coeff = d_coeff_out; a.status = P.max_iters > 0 ? d_st_loop : d_st_final;
    a.phi = c.at<double>(i_ph); a.explicit_t = c.at<double>(i_ex); a.through_p = c.at<double>(i_thp); a.through_t = c.at<double>(i_tht);
    a.fbest = c.at<double>(i_fb); a.alpha = c.at<double>(i_al); a.need = c.at<double>(i_nd); a.sigma = c.at<double>(i_sg);
    a.active = c.at<int32_t>(i_ac);
    a.objective = d_objective_out; a.accepted = d_accepted_out;
    a.ws = P.smooth_weight; a.wt = P.time_weight; a.t_min = P.t_min; a.t_max = P.t_max; a.max_move = P.max_move;
    a.step_move = P.initial_step_move; a.step_log = P.initial_step_log; a.armijo = P.armijo_c; a.shrink = P.shrink; a.grow = P.grow;
    a.propose = P.max_iters > 0 ? 1 : 0;
    q.hist_sp = c.at<double>(i_sp); q.hist_yp = c.at<double>(i_yp); q.hist_su = c.at<double>(i_su); q.hist_yu = c.at<double>(i_yu);
    q.dir_p = c.at<double>(i_dp); q.dir_u = c.at<double>(i_du); q.free_p = c.at<double>(i_fp); q.free_u = c.at<double>(i_fu);
    q.state = c.at<int32_t>(i_state);
    q.wp_len = 3 * (tot + n); q.t_len = tot;
    q.memory = P.memory; q.max_backtracks = P.max_backtracks; q.curvature_eps = P.curvature_eps;
    // the penalty of the point `coeff` was solved at, its two partial gradients, and the coefficient gradient taken through the minimiser to
    // the waypoints and the durations by ONE backward pass
    auto penalty_and_backward = [&](const double* d_wp, const double* d_T, const int32_t* d_st) -> int {
        int e = flight_penalty_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_T, d_coeff_out, d_st, esdf, *limits, *clearance,
                                       c.at<double>(i_ph), c.at<double>(i_g), c.at<double>(i_ex), nullptr, nullptr, nullptr);
        if (e != UAVQP_OK) return e;
        if (with_attitude) {
            e = attitude_penalty_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_T, d_coeff_out, d_st, *attitude, c.at<double>(i_ph),
                                         c.at<double>(i_g), c.at<double>(i_ex), nullptr, true);
            if (e != UAVQP_OK) return e;
        }
        return uavqp_solve_backward_device(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_wp, d_T, d_bc,
                                           d_coeff_out, d_st, c.at<double>(i_g), c.at<double>(i_tht), c.at<double>(i_thp), nullptr);
    };
    const int grid = topt_grid(ctx, n_traj);
    hipStream_t s = ctx->stream;
    auto step = [&](bool init) -> int {
        if (r == 3 && init) hipLaunchKernelGGL((uavqp::spacetime_lbfgs_step_kernel<3, true>), dim3(grid), dim3(64), 0, s, q);
        else if (r == 3) hipLaunchKernelGGL((uavqp::spacetime_lbfgs_step_kernel<3, false>), dim3(grid), dim3(64), 0, s, q);
        else if (init) hipLaunchKernelGGL((uavqp::spacetime_lbfgs_step_kernel<4, true>), dim3(grid), dim3(64), 0, s, q);
        else hipLaunchKernelGGL((uavqp::spacetime_lbfgs_step_kernel<4, false>), dim3(grid), dim3(64), 0, s, q);
        UAVQP_HIP(hipGetLastError());
        return UAVQP_OK;
    };
    // the start is the centre of the box; the trial waypoints start as a copy too, so that the rows no step writes (a trajectory without a
    // segment) are the caller's
    UAVQP_HIP(hipMemcpyAsync(c.at<double>(i_an), d_waypoints, wp_bytes, hipMemcpyDeviceToDevice, s));
    if (P.max_iters > 0) UAVQP_HIP(hipMemcpyAsync(a.wp_trial, d_waypoints, wp_bytes, hipMemcpyDeviceToDevice, s));
    {
        uavqp::TimeOptArgs k;   // (the clamp of the duration optimiser: it reads the span, the durations and the two bounds)
        std::memset(&k, 0, sizeof(k));
        k.n_traj = n_traj; k.uniform = uniform_segments; k.seg_offsets = d_seg_offsets; k.times = d_times; k.t_min = P.t_min; k.t_max = P.t_max;
        if (r == 3) hipLaunchKernelGGL(uavqp::time_opt_clamp_kernel<3>, dim3(grid), dim3(64), 0, s, k);
        else hipLaunchKernelGGL(uavqp::time_opt_clamp_kernel<4>, dim3(grid), dim3(64), 0, s, k);
        UAVQP_HIP(hipGetLastError());
    }
    rc = uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, d_times, d_bc, d_coeff_out,
                                  const_cast<int32_t*>(a.status));
    if (rc != UAVQP_OK) return rc;
    rc = penalty_and_backward(d_waypoints, d_times, a.status);
    if (rc != UAVQP_OK) return rc;
    rc = step(true);
    if (rc != UAVQP_OK) return rc;
    for (int it = 0; it < P.max_iters; ++it) {
        double* d_T = d_trial_t[it & 1];
        rc = uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, a.wp_trial, d_T, d_bc, d_coeff_out, d_st_loop);
        if (rc != UAVQP_OK) return rc;
        rc = penalty_and_backward(a.wp_trial, d_T, d_st_loop);
        if (rc != UAVQP_OK) return rc;
        a.t_eval = d_T; a.t_next = d_trial_t[(it + 1) & 1];
        a.propose = it + 1 < P.max_iters ? 1 : 0;
        rc = step(false);
        if (rc != UAVQP_OK) return rc;
    }
    if (P.max_iters > 0) {
        // the coefficients on return are the solve AT the accepted point (the last trial of a trajectory may have been rejected, and a
        // trajectory that never took part must carry what a plain solve leaves there)
        rc = uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, d_times, d_bc, d_coeff_out,
                                      d_st_final);
        if (rc != UAVQP_OK) return rc;
    }
    if (d_peak_out || d_min_dist_out || d_outside_out)   // the penalty's diagnostics of what is handed back
        rc = flight_penalty_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff_out, d_st_final, esdf, *limits, *clearance,
                                    nullptr, nullptr, nullptr, d_peak_out, d_min_dist_out, d_outside_out);
    if (rc == UAVQP_OK && attitude && d_attitude_peak_out)
        rc = attitude_penalty_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff_out, d_st_final, *attitude, nullptr,
                                      nullptr, nullptr, d_attitude_peak_out);
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

static int spacetime_lbfgs_run_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                    double* waypoints, double* times, const double* bc, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                                    const uavqp_clearance_params* clearance, const uavqp_spacetime_lbfgs_params* params, double* coeff_out,
                                    int32_t* status_out, double* objective_out, int32_t* accepted_out, double* peak_out, double* min_dist_out,
                                    int32_t* outside_out, const uavqp_attitude_params* attitude, double* attitude_peak_out, const char* what) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (!spacetime_lbfgs_params_valid(params) || !limit_params_valid(limits)) return UAVQP_ERR_INVALID_ARG;
    if (!esdf_usable(ctx, esdf) || !esdf->updated || !clearance_params_valid(clearance)) return UAVQP_ERR_INVALID_ARG;
    if (attitude && !attitude_params_valid(attitude)) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!waypoints || !times || !bc || !coeff_out || !objective_out) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && !seg_offsets) return UAVQP_ERR_INVALID_ARG;
    BatchShape sh;
    int rc = batch_shape(n_traj, uniform_segments, max_segments, seg_offsets, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg;
    Stage st;
    const int i_off = uniform_segments > 0 ? -1 : st.in(seg_offsets, sizeof(int32_t) * (n + 1));
    const int i_wp = st.inout(waypoints, sizeof(double) * 3 * (tot + n));
    const int i_t = st.inout(times, sizeof(double) * tot);
    const int i_bc = st.in(bc, sizeof(double) * n * 2 * (r - 1) * 3);
    const int i_out = st.out(coeff_out, sizeof(double) * 3 * 2 * r * tot, true);
    const int i_st = st.out(status_out, sizeof(int32_t) * n);
    const int i_obj = st.out(objective_out, sizeof(double) * 2 * n), i_acc = st.out(accepted_out, sizeof(int32_t) * n);
    const int i_pk = peak_out ? st.out(peak_out, sizeof(double) * 2 * n) : -1;
    const int i_md = min_dist_out ? st.out(min_dist_out, sizeof(double) * n) : -1;
    const int i_o = outside_out ? st.out(outside_out, sizeof(int32_t) * n) : -1;
    const int i_apk = (attitude && attitude_peak_out) ? st.out(attitude_peak_out, sizeof(double) * 4 * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = spacetime_lbfgs_run(ctx, r, n_traj, uniform_segments, sh.Mmax, (int)sh.total_seg, st.at<int32_t>(i_off), st.at<double>(i_wp),
                             st.at<double>(i_t), st.at<double>(i_bc), esdf, limits, clearance, params, st.at<double>(i_out),
                             st.at<int32_t>(i_st), st.at<double>(i_obj), st.at<int32_t>(i_acc), st.at<double>(i_pk), st.at<double>(i_md),
                             st.at<int32_t>(i_o), attitude, st.at<double>(i_apk));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, what);
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
