// uavqp_separation_cert.h -- host side of uavqp_separation_certificate_device / _host (include/uavqp.h): included by uavqp.hip behind
// uavqp_swarm.h, whose description of the swarms and check of their offsets it shares.  Kernel: qp_separation_cert.h
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

// (arguments checked by the callers)
static int separation_cert_enqueue(uavqp_ctx* ctx, const SolvedBatch& B, int n_groups, const int32_t* d_group_offsets, const double* d_start,
                                   const uavqp_separation_params& P, double* d_lower, double* d_upper, int32_t* d_where, int32_t* d_verdict,
                                   int32_t* d_group_verdict) {
    uavqp::SeparationCertArgs a;
    solved_fill(a, B);
    a.n_groups = n_groups; a.group_offsets = d_group_offsets; a.start = d_start;
    a.lower = d_lower; a.upper = d_upper; a.where = d_where; a.verdict = d_verdict; a.group_verdict = d_group_verdict;
    a.n_leaves = P.n_cells << P.depth;
    a.clock_start = P.clock_start; a.h = std::ldexp(P.dt, -P.depth); a.inv_dw = 1.0 / P.downwash; a.d_req = P.d_req;
    // one workgroup per swarm, grid-stride past 2 resident workgroups per CU (the LDS of qp_separation_cert.h)
    const int cap = ctx->separation_cert_blocks > 0 ? ctx->separation_cert_blocks : ctx->num_cus * 2;
    const int grid = n_groups < cap ? n_groups : cap;
    return dispatch_r(B.r, [&](auto R) {
        hipLaunchKernelGGL(uavqp::separation_cert_kernel<decltype(R)::value>, dim3(grid), dim3(uavqp::SEP_BLOCK), 0, ctx->stream, a);
    });
}

extern "C" int uavqp_separation_certificate_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                                   const double* d_times, const double* d_coeff, const int32_t* d_status, int n_groups,
                                                   const int32_t* d_group_offsets, const double* d_start,
                                                   const uavqp_separation_params* params, double* d_lower, double* d_upper, int32_t* d_where,
                                                   int32_t* d_verdict, int32_t* d_group_verdict) {
    const SolvedBatch B{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status};
    bool run;
    const SolvedGroups G{n_groups, d_group_offsets};
    const int rc = solved_args_check(ctx, B, [&] { return separation_params_valid(params); },
                                     d_lower || d_upper || d_where || d_verdict || d_group_verdict, &run, &G);
    if (!run) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return separation_cert_enqueue(ctx, B, n_groups, d_group_offsets, d_start, *params, d_lower, d_upper, d_where, d_verdict, d_group_verdict);
}

extern "C" int uavqp_separation_certificate_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets,
                                                 const double* times, const double* coeff, const int32_t* status, int n_groups,
                                                 const int32_t* group_offsets, const double* start, const uavqp_separation_params* params,
                                                 double* lower, double* upper, int32_t* where, int32_t* verdict, int32_t* group_verdict) {
    const SolvedBatch B{r, n_traj, uniform_segments, seg_offsets, times, coeff, status};
    bool run;
    const SolvedGroups G{n_groups, group_offsets};
    int rc = solved_args_check(ctx, B, [&] { return separation_params_valid(params); },
                               lower || upper || where || verdict || group_verdict, &run, &G);
    if (!run) return rc;
    BatchShape sh;
    rc = swarm_groups_host_check(n_traj, n_groups, group_offsets);
    if (rc == UAVQP_OK) rc = solved_shape(B, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, ng = (size_t)n_groups;
    Stage st;
    SolvedStage in;
    in.declare(st, B, sh);
    const int i_go = group_offsets ? st.in(group_offsets, sizeof(int32_t) * (ng + 1)) : -1;
    const int i_s = start ? st.in(start, sizeof(double) * n) : -1;
    const int i_lo = lower ? st.out(lower, sizeof(double) * n) : -1;
    const int i_up = upper ? st.out(upper, sizeof(double) * n) : -1;
    const int i_w = where ? st.out(where, sizeof(int32_t) * 4 * n) : -1;
    const int i_v = verdict ? st.out(verdict, sizeof(int32_t) * n) : -1;
    const int i_gv = group_verdict ? st.out(group_verdict, sizeof(int32_t) * ng) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = separation_cert_enqueue(ctx, in.device(st), n_groups, st.at<int32_t>(i_go), st.at<double>(i_s), *params, st.at<double>(i_lo),
                                 st.at<double>(i_up), st.at<int32_t>(i_w), st.at<int32_t>(i_v), st.at<int32_t>(i_gv));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_separation_certificate_host");
}
