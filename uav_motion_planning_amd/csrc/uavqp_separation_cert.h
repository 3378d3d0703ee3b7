// uavqp_separation_cert.h -- host side of uavqp_separation_certificate_device / _host (include/uavqp.h): included by uavqp.hip behind
// uavqp_swarm.h, whose description of the swarms it shares; argument check and staging follow that file.  Kernel: qp_separation_cert.h
// (translation unit k_separation_cert.hip).  One launch, nothing allocated (the kernel works in LDS alone), nothing read back.
#pragma once

extern "C" void uavqp_default_separation_params(uavqp_separation_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_separation_params);
    p->depth = 2;         // four leaves per clock cell
    p->n_cells = 64;      // the clock of uavqp_default_swarm_params: 6.4 s of flight
    p->clock_start = 0.0;
    p->dt = 0.1;
    p->downwash = 1.0;
    p->d_req = 1.0;       // the d_safe of uavqp_default_swarm_params
}

static bool separation_params_valid(const uavqp_separation_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_separation_params)) return false;
    if (p->depth < 0 || p->depth > 6 || p->n_cells < 1 || p->n_cells > UAVQP_SEPARATION_MAX_CELLS) return false;
    if (!(p->dt > 0.0 && p->dt < INFINITY) || !(p->d_req > 0.0 && p->d_req < INFINITY)) return false;
    if (!(p->downwash >= 1.0 && p->downwash < INFINITY)) return false;
    if (!(p->clock_start > -INFINITY && p->clock_start < INFINITY)) return false;
    return true;
}

// what both entries refuse before they look at a pointer's contents; *nothing = a valid call with nothing to do
static int separation_args_check(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                                 const double* coeff, int n_groups, const int32_t* group_offsets, const uavqp_separation_params* params,
                                 bool any_out, bool* nothing) {
    *nothing = false;
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || n_groups < 0) return UAVQP_ERR_INVALID_ARG;
    if (!separation_params_valid(params)) return UAVQP_ERR_INVALID_ARG;
    if (!group_offsets && n_groups != 1) return UAVQP_ERR_INVALID_ARG;
    if (n_groups == 0 || !any_out) {
        *nothing = true;
        return UAVQP_OK;
    }
    if (n_traj > 0 && (!times || !coeff || (uniform_segments == 0 && !seg_offsets))) return UAVQP_ERR_INVALID_ARG;
    return UAVQP_OK;
}

// (arguments checked by the callers)
static int separation_cert_enqueue(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets, const double* d_times,
                                   const double* d_coeff, const int32_t* d_status, int n_groups, const int32_t* d_group_offsets,
                                   const double* d_start, const uavqp_separation_params& P, double* d_lower, double* d_upper, int32_t* d_where,
                                   int32_t* d_verdict, int32_t* d_group_verdict) {
    uavqp::SeparationCertArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.n_groups = n_groups; a.seg_offsets = d_seg_offsets; a.group_offsets = d_group_offsets;
    a.times = d_times; a.coeff = d_coeff; a.status = d_status; a.start = d_start;
    a.lower = d_lower; a.upper = d_upper; a.where = d_where; a.verdict = d_verdict; a.group_verdict = d_group_verdict;
    a.n_leaves = P.n_cells << P.depth;
    a.clock_start = P.clock_start; a.h = std::ldexp(P.dt, -P.depth); a.inv_dw = 1.0 / P.downwash; a.d_req = P.d_req;
    // one workgroup per swarm, grid-stride past 2 resident workgroups per CU (the LDS of qp_separation_cert.h)
    const int cap = ctx->separation_cert_blocks > 0 ? ctx->separation_cert_blocks : ctx->num_cus * 2;
    const int grid = n_groups < cap ? n_groups : cap;
    if (r == 3)
        hipLaunchKernelGGL(uavqp::separation_cert_kernel<3>, dim3(grid), dim3(uavqp::SEP_BLOCK), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::separation_cert_kernel<4>, dim3(grid), dim3(uavqp::SEP_BLOCK), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_separation_certificate_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                                   const double* d_times, const double* d_coeff, const int32_t* d_status, int n_groups,
                                                   const int32_t* d_group_offsets, const double* d_start,
                                                   const uavqp_separation_params* params, double* d_lower, double* d_upper, int32_t* d_where,
                                                   int32_t* d_verdict, int32_t* d_group_verdict) {
    bool nothing;
    const int rc = separation_args_check(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, n_groups, d_group_offsets, params,
                                         d_lower || d_upper || d_where || d_verdict || d_group_verdict, &nothing);
    if (rc != UAVQP_OK || nothing) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return separation_cert_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status, n_groups, d_group_offsets,
                                   d_start, *params, d_lower, d_upper, d_where, d_verdict, d_group_verdict);
}

extern "C" int uavqp_separation_certificate_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets,
                                                 const double* times, const double* coeff, const int32_t* status, int n_groups,
                                                 const int32_t* group_offsets, const double* start, const uavqp_separation_params* params,
                                                 double* lower, double* upper, int32_t* where, int32_t* verdict, int32_t* group_verdict) {
    bool nothing;
    int rc = separation_args_check(ctx, r, n_traj, uniform_segments, seg_offsets, times, coeff, n_groups, group_offsets, params,
                                   lower || upper || where || verdict || group_verdict, &nothing);
    if (rc != UAVQP_OK || nothing) return rc;
    // the offsets the device trusts: ascending from 0 to n_traj, no swarm larger than the kernel's lanes
    if (group_offsets) {
        if (group_offsets[0] != 0 || group_offsets[n_groups] != n_traj) return UAVQP_ERR_INVALID_ARG;
        for (int g = 0; g < n_groups; ++g) {
            const long long A = (long long)group_offsets[g + 1] - group_offsets[g];
            if (A < 0 || A > UAVQP_SWARM_MAX_VEHICLES) return UAVQP_ERR_INVALID_ARG;
        }
    } else if (n_traj > UAVQP_SWARM_MAX_VEHICLES) {
        return UAVQP_ERR_INVALID_ARG;
    }
    BatchShape sh{0, 1};
    if (n_traj > 0) {
        rc = batch_shape(n_traj, uniform_segments, 0, seg_offsets, &sh);
        if (rc != UAVQP_OK) return rc;
    }
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg, ng = (size_t)n_groups;
    Stage st;
    const int i_off = (uniform_segments > 0 || n_traj == 0) ? -1 : st.in(seg_offsets, sizeof(int32_t) * (n + 1));
    const int i_t = st.in(times, sizeof(double) * tot);
    const int i_c = st.in(coeff, sizeof(double) * 3 * 2 * r * tot);
    const int i_st = status ? st.in(status, sizeof(int32_t) * n) : -1;
    const int i_go = group_offsets ? st.in(group_offsets, sizeof(int32_t) * (ng + 1)) : -1;
    const int i_s = start ? st.in(start, sizeof(double) * n) : -1;
    const int i_lo = lower ? st.out(lower, sizeof(double) * n) : -1;
    const int i_up = upper ? st.out(upper, sizeof(double) * n) : -1;
    const int i_w = where ? st.out(where, sizeof(int32_t) * 4 * n) : -1;
    const int i_v = verdict ? st.out(verdict, sizeof(int32_t) * n) : -1;
    const int i_gv = group_verdict ? st.out(group_verdict, sizeof(int32_t) * ng) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = separation_cert_enqueue(ctx, r, n_traj, uniform_segments, st.at<int32_t>(i_off), st.at<double>(i_t), st.at<double>(i_c),
                                 st.at<int32_t>(i_st), n_groups, st.at<int32_t>(i_go), st.at<double>(i_s), *params, st.at<double>(i_lo),
                                 st.at<double>(i_up), st.at<int32_t>(i_w), st.at<int32_t>(i_v), st.at<int32_t>(i_gv));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_separation_certificate_host");
}
