// uavqp_waypoint_opt.h -- host side of uavqp_cost_waypoint_gradient_device / _host and uavqp_waypoint_optimize_device / _host
// (include/uavqp.h): included by uavqp.hip behind uavqp_esdf.h, whose penalty it enqueues, uavqp_adjoint.h and uavqp_time_opt.h, whose
// sequencing it shares.  Kernels: qp_waypoint_opt.h (translation unit k_wpopt.hip).
//
// Like the duration optimiser there is NO data-dependent control flow on the host: the number of launches is fixed by max_iters, every
// accept / reject is taken per trajectory on the device, and nothing is read back:
//     anchor copy -> solve(waypoints) -> penalty, backward -> step<INIT>
//       -> max_iters x { solve(trial) -> penalty, backward -> step<ITER> } -> solve(waypoints) -> penalty (min_dist / outside only)
// The inner solve is uavqp_solve_batch_device itself, so the coefficients handed back are those of a plain solve at the waypoints handed back.
#pragma once

extern "C" void uavqp_default_waypoint_opt_params(uavqp_waypoint_opt_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_waypoint_opt_params);
    p->max_iters = 64;        // CPU transcription: at most 4.2 % of L-BFGS-B's decrease left on the test scenes, 7.1 % after 32
    p->smooth_weight = 1.0;
    p->max_move = 2.0;
    p->initial_step = 0.1;    // the first trial moves the most sensitive waypoint component by 10 cm
    p->armijo_c = 1e-4;
    p->shrink = 0.5;
    p->grow = 2.0;
}

static bool wpopt_params_valid(const uavqp_waypoint_opt_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_waypoint_opt_params)) return false;
    if (p->max_iters < 0 || p->max_iters > 100000) return false;
    if (!(p->smooth_weight >= 0.0 && p->smooth_weight < INFINITY)) return false;
    if (!(p->max_move > 0.0)) return false;   // (INFINITY: no box)
    if (!(p->initial_step > 0.0 && p->initial_step < INFINITY)) return false;
    if (!(p->armijo_c > 0.0 && p->armijo_c < 1.0)) return false;
    if (!(p->shrink > 0.0 && p->shrink < 1.0)) return false;
    if (!(p->grow >= 1.0 && p->grow < INFINITY)) return false;
    return true;
}

extern "C" int uavqp_cost_waypoint_gradient_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                                   const double* d_coeff, const int32_t* d_status, double* d_grad) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0 || !d_grad) return UAVQP_OK;
    if (!d_coeff || (uniform_segments == 0 && !d_seg_offsets)) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    uavqp::WaypointGradArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.seg_offsets = d_seg_offsets; a.coeff = d_coeff; a.status = d_status; a.grad = d_grad;
    const int grid = topt_grid(ctx, n_traj);
    if (r == 3)
        hipLaunchKernelGGL(uavqp::cost_waypoint_grad_kernel<3>, dim3(grid), dim3(64), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::cost_waypoint_grad_kernel<4>, dim3(grid), dim3(64), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_cost_waypoint_gradient_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets,
                                                 const double* coeff, const int32_t* status, double* grad) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0 || !grad) return UAVQP_OK;
    if (!coeff || (uniform_segments == 0 && !seg_offsets)) return UAVQP_ERR_INVALID_ARG;
    BatchShape sh;
    int rc = batch_shape(n_traj, uniform_segments, 0, seg_offsets, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg;
    Stage st;
    const int i_off = uniform_segments > 0 ? -1 : st.in(seg_offsets, sizeof(int32_t) * (n + 1));
    const int i_c = st.in(coeff, sizeof(double) * 3 * 2 * r * tot);
    const int i_st = status ? st.in(status, sizeof(int32_t) * n) : -1;
    const int i_g = st.out(grad, sizeof(double) * 3 * (tot + n));
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = uavqp_cost_waypoint_gradient_device(ctx, r, n_traj, uniform_segments, st.at<int32_t>(i_off), st.at<double>(i_c), st.at<int32_t>(i_st),
                                             st.at<double>(i_g));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_cost_waypoint_gradient_host");
}

extern "C" int uavqp_waypoint_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                              const int32_t* d_seg_offsets, double* d_waypoints, const double* d_times, const double* d_bc,
                                              const uavqp_esdf* esdf, const uavqp_clearance_params* clearance,
                                              const uavqp_waypoint_opt_params* params, double* d_coeff_out, int32_t* d_status_out,
                                              double* d_objective_out, int32_t* d_accepted_out, double* d_min_dist_out, int32_t* d_outside_out) {
    bool run;
    int rc = descent_args_check(ctx, r, n_traj, 1, uniform_segments, max_segments, total_segments, d_seg_offsets,
                                d_waypoints && d_times && d_bc && d_coeff_out && d_objective_out, true, [&] {
                                    return wpopt_params_valid(params) && esdf_usable(ctx, esdf) && esdf->updated && clearance_params_valid(clearance);
                                }, &run);
    if (!run) return rc;
    const uavqp_waypoint_opt_params P = *params;
    const size_t n = (size_t)n_traj, tot = (size_t)total_segments, wp_bytes = sizeof(double) * 3 * (tot + n);

    Carve c;
    const int i_tr = c.add(wp_bytes), i_an = c.add(wp_bytes), i_gb = c.add(wp_bytes), i_g = c.add(sizeof(double) * 3 * 2 * r * tot);
    const int i_th = c.add(wp_bytes), i_ph = c.add(sizeof(double) * n), i_fb = c.add(sizeof(double) * n), i_al = c.add(sizeof(double) * n);
    const int i_nd = c.add(sizeof(double) * n), i_ac = c.add(sizeof(int32_t) * n), i_st = c.add(sizeof(int32_t) * n);
    rc = carve_on(ctx->stream, ctx->topt, c);
    if (rc != UAVQP_OK) return rc;
    int32_t* d_st_loop = c.at<int32_t>(i_st);
    int32_t* d_st_final = d_status_out ? d_status_out : d_st_loop;

    uavqp::WaypointOptArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.seg_offsets = d_seg_offsets;
    a.waypoints = d_waypoints; a.trial = c.at<double>(i_tr); a.anchor = c.at<double>(i_an); a.gbest = c.at<double>(i_gb);
    a.times = d_times; a.coeff = d_coeff_out;
    a.phi = c.at<double>(i_ph); a.through = c.at<double>(i_th);
    a.fbest = c.at<double>(i_fb); a.alpha = c.at<double>(i_al); a.need = c.at<double>(i_nd); a.active = c.at<int32_t>(i_ac);
    a.objective = d_objective_out; a.accepted = d_accepted_out;
    a.ws = P.smooth_weight; a.max_move = P.max_move; a.initial_step = P.initial_step; a.armijo = P.armijo_c; a.shrink = P.shrink; a.grow = P.grow;
    const int grid = topt_grid(ctx, n_traj);
    hipStream_t s = ctx->stream;
    // the waypoints and the status of a point of the sequence; the step kernel reads the status of the solve before it
    auto waypoints_at = [&](const DescentPoint& p) { return p.at == DescentAt::TRIAL ? a.trial : d_waypoints; };
    auto solved = [&](const int32_t* st) { return SolvedBatch{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff_out, st}; };
    auto solve = [&](const DescentPoint& p) -> int {
        a.status = p.caller_status ? d_st_final : d_st_loop;
        return uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, waypoints_at(p), d_times, d_bc, d_coeff_out,
                                        const_cast<int32_t*>(a.status));
    };
    // the penalty of the point `coeff` was solved at, its gradient in the coefficients, and that gradient taken through the minimiser to the waypoints
    auto penalty_and_backward = [&](const DescentPoint& p) -> int {
        int e = clearance_penalty_enqueue(ctx, solved(a.status), esdf, *clearance, c.at<double>(i_ph), c.at<double>(i_g), nullptr, nullptr, nullptr);
        if (e != UAVQP_OK) return e;
        return uavqp_solve_backward_device(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, waypoints_at(p), d_times,
                                           d_bc, d_coeff_out, a.status, c.at<double>(i_g), nullptr, c.at<double>(i_th), nullptr);
    };
    auto step = [&](bool init, int, bool propose) -> int {
        a.propose = propose ? 1 : 0;
        return dispatch_r_flag(r, init, [&](auto R, auto INIT) {
            hipLaunchKernelGGL((uavqp::waypoint_opt_step_kernel<decltype(R)::value, decltype(INIT)::value>), dim3(grid), dim3(64), 0, s, a);
        });
    };
    // the start is the centre of the box; the trial array starts as a copy too, so that the rows no step writes (a trajectory without a
    // segment) are the caller's
    UAVQP_HIP(hipMemcpyAsync(c.at<double>(i_an), d_waypoints, wp_bytes, hipMemcpyDeviceToDevice, s));
    if (P.max_iters > 0) UAVQP_HIP(hipMemcpyAsync(a.trial, d_waypoints, wp_bytes, hipMemcpyDeviceToDevice, s));
    rc = descent_sequence(P.max_iters, solve, penalty_and_backward, step);
    if (rc != UAVQP_OK) return rc;
    if (d_min_dist_out || d_outside_out)   // the penalty's diagnostics of what is handed back
        rc = clearance_penalty_enqueue(ctx, solved(d_st_final), esdf, *clearance, nullptr, nullptr, nullptr, d_min_dist_out, d_outside_out);
    return rc;
}

extern "C" int uavqp_waypoint_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                            double* waypoints, const double* times, const double* bc, const uavqp_esdf* esdf,
                                            const uavqp_clearance_params* clearance, const uavqp_waypoint_opt_params* params, double* coeff_out,
                                            int32_t* status_out, double* objective_out, int32_t* accepted_out, double* min_dist_out,
                                            int32_t* outside_out) {
    return descent_run_host(
        ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, waypoints, times, nullptr, bc,
        [&] { return wpopt_params_valid(params) && esdf_usable(ctx, esdf) && esdf->updated && clearance_params_valid(clearance); }, coeff_out,
        status_out, objective_out, accepted_out, nullptr, min_dist_out, outside_out, nullptr, 0, "uavqp_waypoint_optimize_host",
        [&](const DescentStaged& d) {
            return uavqp_waypoint_optimize_device(ctx, r, n_traj, uniform_segments, d.Mmax, d.total_segments, d.seg_offsets, d.waypoints, d.times,
                                                  d.bc, esdf, clearance, params, d.coeff, d.status, d.objective, d.accepted, d.min_dist, d.outside);
        });
}
