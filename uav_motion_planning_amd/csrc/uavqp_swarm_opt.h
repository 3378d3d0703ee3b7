// uavqp_swarm_opt.h -- host side of uavqp_swarm_optimize_device / _host (include/uavqp.h): included by uavqp.hip behind uavqp_spacetime.h
// and uavqp_swarm.h, whose parameter checks and enqueue helpers it shares.  Kernels: qp_swarm_opt.h (translation unit k_swarm_opt.hip).
//
// The sequencing of uavqp_spacetime_optimize_device with the swarm penalty between the flight penalty and the backward pass.  NO
// data-dependent control flow on the host, nothing read back; every accept / reject is taken per SWARM on the device:
//     anchor copies -> clamp -> solve(waypoints, times) -> flight penalty -> swarm penalty (accumulating) -> backward -> step<INIT>
//       -> max_iters x { solve(trial waypoints, trial durations) -> flight penalty -> swarm penalty at the trial departures (accumulating)
//                        -> backward -> step<ITER> }
//       -> solve(waypoints, times) -> flight penalty (peak / min_dist / outside only) -> swarm penalty (min_sep only)
// Five launches per trial.  The swarm penalty ADDS its dPhi/dc and explicit dPhi/dT to what the flight penalty has just written (every
// element has one owning lane in either kernel), so ONE backward pass takes the sum through the minimiser.
#pragma once

extern "C" void uavqp_default_swarm_opt_params(uavqp_swarm_opt_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    uavqp_spacetime_params s;
    uavqp_default_spacetime_params(&s);
    p->struct_size = (int32_t)sizeof(uavqp_swarm_opt_params);
    p->max_iters = s.max_iters;
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
    p->start_window = 0.0;          // the departures are fixed
    p->initial_step_start = 0.1;    // the first trial moves the most sensitive departure by 0.1 s
}

static bool swarm_opt_params_valid(const uavqp_swarm_opt_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_swarm_opt_params)) return false;
    const uavqp_spacetime_params s = spacetime_part_of(*p);
    if (!spacetime_params_valid(&s)) return false;
    if (!(p->start_window >= 0.0 && p->start_window < INFINITY)) return false;
    if (!(p->initial_step_start > 0.0 && p->initial_step_start < INFINITY)) return false;
    return true;
}

extern "C" int uavqp_swarm_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                           const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc,
                                           int n_groups, const int32_t* d_group_offsets, double* d_start, const uavqp_esdf* esdf,
                                           const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                           const uavqp_swarm_params* swarm, const uavqp_swarm_opt_params* params, double* d_coeff_out,
                                           int32_t* d_status_out, double* d_objective_out, int32_t* d_accepted_out, double* d_peak_out,
                                           double* d_min_dist_out, int32_t* d_outside_out, double* d_min_sep_out) {
    bool run;
    int rc = descent_args_check(ctx, r, n_traj, n_groups, uniform_segments, max_segments, total_segments, d_seg_offsets,
                                d_waypoints && d_times && d_bc && d_coeff_out && d_objective_out, true, [&] {
                                    return swarm_opt_params_valid(params) && swarm_params_valid(swarm) &&
                                           flight_params_valid(ctx, esdf, limits, clearance) && (d_group_offsets || n_groups == 1) &&
                                           (d_start || !(params->start_window > 0.0));
                                }, &run);
    if (!run) return rc;
    const uavqp_swarm_opt_params P = *params;
    const size_t n = (size_t)n_traj, ng = (size_t)n_groups, s_bytes = sizeof(double) * n;
    const bool starts = d_start != nullptr;

    JointRun j{ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_times, d_bc, esdf, limits, clearance,
               d_coeff_out, d_status_out};
    Carve& c = j.c;
    j.k.declare(c, r, n, (size_t)total_segments);
    const int i_str = c.add(s_bytes, starts), i_san = c.add(s_bytes, starts), i_gs = c.add(s_bytes, starts), i_gsb = c.add(s_bytes, starts);
    const int i_phs = c.add(sizeof(double) * ng), i_fb = c.add(sizeof(double) * ng), i_al = c.add(sizeof(double) * ng);
    const int i_nd = c.add(sizeof(double) * ng), i_sg = c.add(sizeof(double) * 3 * ng), i_ga = c.add(sizeof(int32_t) * ng);
    rc = carve_on(ctx->stream, ctx->topt, c);
    if (rc != UAVQP_OK) return rc;

    uavqp::SwarmOptArgs a;
    j.fill(a, P, d_objective_out, d_accepted_out);
    a.n_groups = n_groups; a.group_offsets = d_group_offsets;
    a.start = d_start; a.start_trial = c.at<double>(i_str); a.start_anchor = c.at<double>(i_san); a.grad_start = c.at<double>(i_gs);
    a.gs_best = c.at<double>(i_gsb);
    a.phi_swarm = c.at<double>(i_phs); a.fbest = c.at<double>(i_fb); a.alpha = c.at<double>(i_al); a.need = c.at<double>(i_nd);
    a.sigma = c.at<double>(i_sg); a.g_active = c.at<int32_t>(i_ga);
    a.window = P.start_window; a.step_start = P.initial_step_start;
    // the swarm penalty at the departures of the point `coeff` was solved at ADDS to what the flight penalty has just written: the sum of
    // the partial gradients in ONE pair of arrays, for ONE backward pass
    auto swarm_penalty = [&](const DescentPoint& p) -> int {
        const double* d_s = p.at == DescentAt::TRIAL ? a.start_trial : d_start;   // (null without departures, either way)
        return swarm_penalty_enqueue(ctx, j.solved_at(p), n_groups, d_group_offsets, d_s, *swarm, c.at<double>(i_phs), j.at<double>(j.k.g),
                                     j.at<double>(j.k.ex), c.at<double>(i_gs), nullptr, true);
    };
    // one workgroup per swarm, grid-stride past eight resident workgroups per CU
    const int cap = ctx->num_cus * 8;
    const int grid = n_groups < cap ? n_groups : cap;
    hipStream_t s = ctx->stream;
    // the start is the centre of the box and of the window; the trial waypoints and departures start as copies too, so that what no step
    // writes (a trajectory without a segment, a vehicle outside every swarm) is the caller's
    rc = j.anchor_copies(P.max_iters);
    if (rc != UAVQP_OK) return rc;
    if (starts) {
        UAVQP_HIP(hipMemcpyAsync(c.at<double>(i_san), d_start, s_bytes, hipMemcpyDeviceToDevice, s));
        UAVQP_HIP(hipMemcpyAsync(a.start_trial, d_start, s_bytes, hipMemcpyDeviceToDevice, s));
    }
    rc = time_clamp_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, P.t_min, P.t_max);
    if (rc == UAVQP_OK)
        rc = j.descend(a, P.max_iters, swarm_penalty, [&](auto R, auto INIT) {
            hipLaunchKernelGGL((uavqp::swarm_step_kernel<decltype(R)::value, decltype(INIT)::value>), dim3(grid), dim3(uavqp::SWOPT_BLOCK), 0, s, a);
        });
    if (rc == UAVQP_OK) rc = j.flight_diagnostics(d_peak_out, d_min_dist_out, d_outside_out);   // the penalties' diagnostics of what is handed back
    if (rc == UAVQP_OK && d_min_sep_out)
        rc = swarm_penalty_enqueue(ctx, j.solved_final(), n_groups, d_group_offsets, d_start, *swarm, nullptr, nullptr, nullptr, nullptr,
                                   d_min_sep_out);
    return rc;
}

extern "C" int uavqp_swarm_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                         double* waypoints, double* times, const double* bc, int n_groups, const int32_t* group_offsets,
                                         double* start, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                                         const uavqp_clearance_params* clearance, const uavqp_swarm_params* swarm,
                                         const uavqp_swarm_opt_params* params, double* coeff_out, int32_t* status_out, double* objective_out,
                                         int32_t* accepted_out, double* peak_out, double* min_dist_out, int32_t* outside_out,
                                         double* min_sep_out) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || n_groups < 0) return UAVQP_ERR_INVALID_ARG;
    if (!swarm_opt_params_valid(params) || !swarm_params_valid(swarm)) return UAVQP_ERR_INVALID_ARG;
    if (!flight_params_valid(ctx, esdf, limits, clearance)) return UAVQP_ERR_INVALID_ARG;
    if (!group_offsets && n_groups != 1) return UAVQP_ERR_INVALID_ARG;
    if (params->start_window > 0.0 && !start) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0 || n_groups == 0) return UAVQP_OK;
    if (!waypoints || !times || !bc || !coeff_out || !objective_out) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && !seg_offsets) return UAVQP_ERR_INVALID_ARG;
    // the offsets the device trusts: ascending from 0 to n_traj, no swarm larger than the kernels' lanes
    if (group_offsets) {
        if (group_offsets[0] != 0 || group_offsets[n_groups] != n_traj) return UAVQP_ERR_INVALID_ARG;
        for (int g = 0; g < n_groups; ++g) {
            const long long A = (long long)group_offsets[g + 1] - group_offsets[g];
            if (A < 0 || A > UAVQP_SWARM_MAX_VEHICLES) return UAVQP_ERR_INVALID_ARG;
        }
    } else if (n_traj > UAVQP_SWARM_MAX_VEHICLES) {
        return UAVQP_ERR_INVALID_ARG;
    }
    BatchShape sh;
    int rc = batch_shape(n_traj, uniform_segments, max_segments, seg_offsets, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg, ng = (size_t)n_groups;
    Stage st;
    const int i_off = uniform_segments > 0 ? -1 : st.in(seg_offsets, sizeof(int32_t) * (n + 1));
    const int i_wp = st.inout(waypoints, sizeof(double) * 3 * (tot + n));
    const int i_t = st.inout(times, sizeof(double) * tot);
    const int i_bc = st.in(bc, sizeof(double) * n * 2 * (r - 1) * 3);
    const int i_go = group_offsets ? st.in(group_offsets, sizeof(int32_t) * (ng + 1)) : -1;
    const int i_s = start ? st.inout(start, sizeof(double) * n) : -1;
    const int i_out = st.out(coeff_out, sizeof(double) * 3 * 2 * r * tot, true);
    const int i_st = st.out(status_out, sizeof(int32_t) * n);
    const int i_obj = st.out(objective_out, sizeof(double) * 2 * ng), i_acc = st.out(accepted_out, sizeof(int32_t) * ng);
    const int i_pk = peak_out ? st.out(peak_out, sizeof(double) * 2 * n) : -1;
    const int i_md = min_dist_out ? st.out(min_dist_out, sizeof(double) * n) : -1;
    const int i_o = outside_out ? st.out(outside_out, sizeof(int32_t) * n) : -1;
    const int i_ms = min_sep_out ? st.out(min_sep_out, sizeof(double) * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = uavqp_swarm_optimize_device(ctx, r, n_traj, uniform_segments, sh.Mmax, (int)sh.total_seg, st.at<int32_t>(i_off), st.at<double>(i_wp),
                                     st.at<double>(i_t), st.at<double>(i_bc), n_groups, st.at<int32_t>(i_go), st.at<double>(i_s), esdf, limits,
                                     clearance, swarm, params, st.at<double>(i_out), st.at<int32_t>(i_st), st.at<double>(i_obj),
                                     st.at<int32_t>(i_acc), st.at<double>(i_pk), st.at<double>(i_md), st.at<int32_t>(i_o), st.at<double>(i_ms));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_swarm_optimize_host");
}
