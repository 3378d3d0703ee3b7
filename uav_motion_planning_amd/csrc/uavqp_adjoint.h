// uavqp_adjoint.h -- host side of uavqp_solve_backward_device / _host (include/uavqp.h): included by uavqp.hip behind the entry points of the
// duration optimiser.  Kernel: qp_adjoint.h (translation unit k_adjoint.hip).  One launch, nothing read back, no data-dependent control flow.
#pragma once

extern "C" int uavqp_solve_backward_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                           const int32_t* d_seg_offsets, const double* d_waypoints, const double* d_times, const double* d_bc,
                                           const double* d_coeff, const int32_t* d_status, const double* d_grad_coeff, double* d_grad_times,
                                           double* d_grad_waypoints, double* d_grad_bc) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || total_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0 || (!d_grad_times && !d_grad_waypoints && !d_grad_bc)) return UAVQP_OK;
    if (!d_waypoints || !d_times || !d_bc || !d_coeff || !d_grad_coeff) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && (!d_seg_offsets || max_segments < 1)) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments > 0 && (long long)total_segments != (long long)uniform_segments * n_traj) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const int Mmax = uniform_segments > 0 ? uniform_segments : max_segments;
    // one lane per trajectory; the sweep state is per RESIDENT lane (Mmax * F doubles each), so the cap on the grid is a cap on the workspace:
    // 8 * Mmax * F * 128 * num_cus bytes (r = 4, 24 segments, 256 CUs: 138 MB) however large the batch; larger batches stride over it
    int grid = (n_traj + 63) / 64;
    const int max_grid = ctx->num_cus * 2;
    if (grid > max_grid) grid = max_grid;
    const int F = r == 3 ? uavqp::AdjointRec<3>::F : uavqp::AdjointRec<4>::F;
    Carve c;
    const int i_ws = c.add(sizeof(double) * (size_t)Mmax * F * (size_t)grid * 64);
    const int rc = carve_on(ctx->stream, ctx->ws, c);
    if (rc != UAVQP_OK) return rc;
    uavqp::AdjointArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.max_segments = Mmax; a.seg_offsets = d_seg_offsets;
    a.waypoints = d_waypoints; a.times = d_times; a.bc = d_bc; a.coeff = d_coeff; a.status = d_status; a.grad_coeff = d_grad_coeff;
    a.grad_times = d_grad_times; a.grad_waypoints = d_grad_waypoints; a.grad_bc = d_grad_bc;
    a.ws = c.at<double>(i_ws);
    if (r == 3)
        hipLaunchKernelGGL(uavqp::solve_backward_kernel<3>, dim3(grid), dim3(64), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::solve_backward_kernel<4>, dim3(grid), dim3(64), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_solve_backward_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                         const double* waypoints, const double* times, const double* bc, const double* coeff,
                                         const int32_t* status, const double* grad_coeff, double* grad_times, double* grad_waypoints,
                                         double* grad_bc) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0 || (!grad_times && !grad_waypoints && !grad_bc)) return UAVQP_OK;
    if (!waypoints || !times || !bc || !coeff || !grad_coeff) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && !seg_offsets) return UAVQP_ERR_INVALID_ARG;
    BatchShape sh;
    int rc = batch_shape(n_traj, uniform_segments, max_segments, seg_offsets, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg;
    Stage st;
    const int i_off = uniform_segments > 0 ? -1 : st.in(seg_offsets, sizeof(int32_t) * (n + 1));
    const int i_wp = st.in(waypoints, sizeof(double) * 3 * (tot + n));
    const int i_t = st.in(times, sizeof(double) * tot);
    const int i_bc = st.in(bc, sizeof(double) * n * 2 * (r - 1) * 3);
    const int i_c = st.in(coeff, sizeof(double) * 3 * 2 * r * tot);
    const int i_st = status ? st.in(status, sizeof(int32_t) * n) : -1;
    const int i_g = st.in(grad_coeff, sizeof(double) * 3 * 2 * r * tot);
    // (cleared: the kernel writes every element of a trajectory it can address; one whose offsets are out of order is not addressed at all)
    const int i_gt = grad_times ? st.out(grad_times, sizeof(double) * tot, true) : -1;
    const int i_gw = grad_waypoints ? st.out(grad_waypoints, sizeof(double) * 3 * (tot + n), true) : -1;
    const int i_gb = grad_bc ? st.out(grad_bc, sizeof(double) * n * 2 * (r - 1) * 3, true) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = uavqp_solve_backward_device(ctx, r, n_traj, uniform_segments, sh.Mmax, (int)sh.total_seg, st.at<int32_t>(i_off), st.at<double>(i_wp),
                                     st.at<double>(i_t), st.at<double>(i_bc), st.at<double>(i_c), st.at<int32_t>(i_st), st.at<double>(i_g),
                                     st.at<double>(i_gt), st.at<double>(i_gw), st.at<double>(i_gb));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_solve_backward_host");
}
