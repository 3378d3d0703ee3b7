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
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || total_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (!wpopt_params_valid(params)) return UAVQP_ERR_INVALID_ARG;
    if (!esdf_usable(ctx, esdf) || !esdf->updated || !clearance_params_valid(clearance)) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!d_waypoints || !d_times || !d_bc || !d_coeff_out || !d_objective_out) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && (!d_seg_offsets || max_segments < 1)) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments > 0 && (long long)total_segments != (long long)uniform_segments * n_traj) return UAVQP_ERR_INVALID_ARG;
    if ((long long)total_segments > 0x7fffffffLL - n_traj) return UAVQP_ERR_INVALID_ARG;   // (the waypoint rows are counted in ints)
    UAVQP_HIP(hipSetDevice(ctx->device));
    const uavqp_waypoint_opt_params P = *params;
    const size_t n = (size_t)n_traj, tot = (size_t)total_segments, wp_bytes = sizeof(double) * 3 * (tot + n);

    Carve c;
    const int i_tr = c.add(wp_bytes), i_an = c.add(wp_bytes), i_gb = c.add(wp_bytes), i_g = c.add(sizeof(double) * 3 * 2 * r * tot);
    const int i_th = c.add(wp_bytes), i_ph = c.add(sizeof(double) * n), i_fb = c.add(sizeof(double) * n), i_al = c.add(sizeof(double) * n);
    const int i_nd = c.add(sizeof(double) * n), i_ac = c.add(sizeof(int32_t) * n), i_st = c.add(sizeof(int32_t) * n);
    int rc = carve_on(ctx->stream, ctx->topt, c);
    if (rc != UAVQP_OK) return rc;
    int32_t* d_st_loop = c.at<int32_t>(i_st);
    int32_t* d_st_final = d_status_out ? d_status_out : d_st_loop;

    uavqp::WaypointOptArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.seg_offsets = d_seg_offsets;
    a.waypoints = d_waypoints; a.trial = c.at<double>(i_tr); a.anchor = c.at<double>(i_an); a.gbest = c.at<double>(i_gb);
    a.times = d_times; a.coeff = d_coeff_out; a.status = P.max_iters > 0 ? d_st_loop : d_st_final;
    a.phi = c.at<double>(i_ph); a.through = c.at<double>(i_th);
    a.fbest = c.at<double>(i_fb); a.alpha = c.at<double>(i_al); a.need = c.at<double>(i_nd); a.active = c.at<int32_t>(i_ac);
    a.objective = d_objective_out; a.accepted = d_accepted_out;
    a.ws = P.smooth_weight; a.max_move = P.max_move; a.initial_step = P.initial_step; a.armijo = P.armijo_c; a.shrink = P.shrink; a.grow = P.grow;
    a.propose = P.max_iters > 0 ? 1 : 0;
    // the penalty of the point `coeff` was solved at, its gradient in the coefficients, and that gradient taken through the minimiser to the waypoints
    auto penalty_and_backward = [&](const double* d_wp, const int32_t* d_st) -> int {
        int e = clearance_penalty_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff_out, d_st, esdf, *clearance,
                                          c.at<double>(i_ph), c.at<double>(i_g), nullptr, nullptr, nullptr);
        if (e != UAVQP_OK) return e;
        return uavqp_solve_backward_device(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_wp, d_times, d_bc,
                                           d_coeff_out, d_st, c.at<double>(i_g), nullptr, c.at<double>(i_th), nullptr);
    };
    const int grid = topt_grid(ctx, n_traj);
    hipStream_t s = ctx->stream;
    auto step = [&](bool init) -> int {
        if (r == 3 && init) hipLaunchKernelGGL((uavqp::waypoint_opt_step_kernel<3, true>), dim3(grid), dim3(64), 0, s, a);
        else if (r == 3) hipLaunchKernelGGL((uavqp::waypoint_opt_step_kernel<3, false>), dim3(grid), dim3(64), 0, s, a);
        else if (init) hipLaunchKernelGGL((uavqp::waypoint_opt_step_kernel<4, true>), dim3(grid), dim3(64), 0, s, a);
        else hipLaunchKernelGGL((uavqp::waypoint_opt_step_kernel<4, false>), dim3(grid), dim3(64), 0, s, a);
        UAVQP_HIP(hipGetLastError());
        return UAVQP_OK;
    };
    // the start is the centre of the box; the trial array starts as a copy too, so that the rows no step writes (a trajectory without a
    // segment) are the caller's
    UAVQP_HIP(hipMemcpyAsync(c.at<double>(i_an), d_waypoints, wp_bytes, hipMemcpyDeviceToDevice, s));
    if (P.max_iters > 0) UAVQP_HIP(hipMemcpyAsync(a.trial, d_waypoints, wp_bytes, hipMemcpyDeviceToDevice, s));
    rc = uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, d_times, d_bc, d_coeff_out,
                                  const_cast<int32_t*>(a.status));
    if (rc != UAVQP_OK) return rc;
    rc = penalty_and_backward(d_waypoints, a.status);
    if (rc != UAVQP_OK) return rc;
    rc = step(true);
    if (rc != UAVQP_OK) return rc;
    for (int it = 0; it < P.max_iters; ++it) {
        rc = uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, a.trial, d_times, d_bc, d_coeff_out, d_st_loop);
        if (rc != UAVQP_OK) return rc;
        rc = penalty_and_backward(a.trial, d_st_loop);
        if (rc != UAVQP_OK) return rc;
        a.propose = it + 1 < P.max_iters ? 1 : 0;
        rc = step(false);
        if (rc != UAVQP_OK) return rc;
    }
    if (P.max_iters > 0) {
        // the coefficients on return are the solve AT the accepted waypoints (the last trial of a trajectory may have been rejected, and a
        // trajectory that never took part must carry what a plain solve leaves there)
        rc = uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, d_times, d_bc, d_coeff_out,
                                      d_st_final);
        if (rc != UAVQP_OK) return rc;
    }
    if (d_min_dist_out || d_outside_out)   // the penalty's diagnostics of what is handed back
        rc = clearance_penalty_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff_out, d_st_final, esdf, *clearance, nullptr,
                                       nullptr, nullptr, d_min_dist_out, d_outside_out);
    return rc;
}

extern "C" int uavqp_waypoint_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                            double* waypoints, const double* times, const double* bc, const uavqp_esdf* esdf,
                                            const uavqp_clearance_params* clearance, const uavqp_waypoint_opt_params* params, double* coeff_out,
                                            int32_t* status_out, double* objective_out, int32_t* accepted_out, double* min_dist_out,
                                            int32_t* outside_out) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (!wpopt_params_valid(params)) return UAVQP_ERR_INVALID_ARG;
    if (!esdf_usable(ctx, esdf) || !esdf->updated || !clearance_params_valid(clearance)) return UAVQP_ERR_INVALID_ARG;
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
    const int i_t = st.in(times, sizeof(double) * tot);
    const int i_bc = st.in(bc, sizeof(double) * n * 2 * (r - 1) * 3);
    const int i_out = st.out(coeff_out, sizeof(double) * 3 * 2 * r * tot, true);
    const int i_st = st.out(status_out, sizeof(int32_t) * n);
    const int i_obj = st.out(objective_out, sizeof(double) * 2 * n), i_acc = st.out(accepted_out, sizeof(int32_t) * n);
    const int i_md = min_dist_out ? st.out(min_dist_out, sizeof(double) * n) : -1;
    const int i_o = outside_out ? st.out(outside_out, sizeof(int32_t) * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = uavqp_waypoint_optimize_device(ctx, r, n_traj, uniform_segments, sh.Mmax, (int)sh.total_seg, st.at<int32_t>(i_off), st.at<double>(i_wp),
                                        st.at<double>(i_t), st.at<double>(i_bc), esdf, clearance, params, st.at<double>(i_out),
                                        st.at<int32_t>(i_st), st.at<double>(i_obj), st.at<int32_t>(i_acc), st.at<double>(i_md),
                                        st.at<int32_t>(i_o));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_waypoint_optimize_host");
}
