// uavqp_swarm.h -- host side of uavqp_swarm_penalty_device / _host (include/uavqp.h): included by uavqp.hip behind uavqp_stage.h.
// Kernel: qp_swarm.h (translation unit k_swarm.hip).  One launch, nothing allocated (the kernel works in LDS alone), nothing read back.
#pragma once

extern "C" void uavqp_default_swarm_params(uavqp_swarm_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_swarm_params);
    p->n_samples = 64;
    p->clock_start = 0.0;
    p->dt = 0.1;          // 64 samples: 6.4 s of flight
    p->d_safe = 1.0;
    p->downwash = 1.0;
    p->weight = 1e3;      // comparable with the other penalties: x is dimensionless
}

static bool swarm_params_valid(const uavqp_swarm_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_swarm_params)) return false;
    if (p->n_samples < 1) return false;
    if (!(p->dt > 0.0 && p->dt < INFINITY) || !(p->d_safe > 0.0 && p->d_safe < INFINITY)) return false;
    if (!(p->downwash >= 1.0 && p->downwash < INFINITY)) return false;
    if (!(p->weight >= 0.0 && p->weight < INFINITY)) return false;
    if (!(p->clock_start > -INFINITY && p->clock_start < INFINITY)) return false;
    return true;
}

// What the _host swarm entries (this file, uavqp_separation_cert.h) check in the offsets the device trusts: ascending from 0 to n_traj,
// no swarm larger than the kernel's lanes.
static int swarm_groups_host_check(int n_traj, int n_groups, const int32_t* group_offsets) {
    if (!group_offsets) return n_traj > UAVQP_SWARM_MAX_VEHICLES ? UAVQP_ERR_INVALID_ARG : UAVQP_OK;
    if (group_offsets[0] != 0 || group_offsets[n_groups] != n_traj) return UAVQP_ERR_INVALID_ARG;
    for (int g = 0; g < n_groups; ++g) {
        const long long A = (long long)group_offsets[g + 1] - group_offsets[g];
        if (A < 0 || A > UAVQP_SWARM_MAX_VEHICLES) return UAVQP_ERR_INVALID_ARG;
    }
    return UAVQP_OK;
}

// (arguments checked by the callers)  accumulate (uavqp_swarm_opt.h only, not in the C ABI): grad_coeff and grad_times are ADDED to what
// the arrays hold
static int swarm_penalty_enqueue(uavqp_ctx* ctx, const SolvedBatch& B, int n_groups, const int32_t* d_group_offsets, const double* d_start,
                                 const uavqp_swarm_params& S, double* d_penalty, double* d_grad_coeff, double* d_grad_times, double* d_grad_start,
                                 double* d_min_sep, bool accumulate = false) {
    uavqp::SwarmArgs a;
    solved_fill(a, B);
    a.n_groups = n_groups; a.group_offsets = d_group_offsets; a.start = d_start;
    a.penalty = d_penalty; a.grad_coeff = d_grad_coeff; a.grad_times = d_grad_times; a.grad_start = d_grad_start; a.min_sep = d_min_sep;
    a.N = S.n_samples; a.clock_start = S.clock_start; a.dt = S.dt; a.d_safe = S.d_safe;
    a.inv_d2 = 1.0 / (S.d_safe * S.d_safe); a.inv_dw2 = 1.0 / (S.downwash * S.downwash);
    a.weight = S.weight; a.force = -6.0 * S.weight * a.inv_d2;
    // one workgroup per swarm, grid-stride past 5 resident workgroups per CU (the LDS of qp_swarm.h)
    const int cap = ctx->num_cus * 5;
    const int grid = n_groups < cap ? n_groups : cap;
    return dispatch_r_flag(B.r, accumulate, [&](auto R, auto ACC) {
        hipLaunchKernelGGL((uavqp::swarm_penalty_kernel<decltype(R)::value, decltype(ACC)::value>), dim3(grid), dim3(uavqp::SWARM_BLOCK), 0,
                           ctx->stream, a);
    });
}

extern "C" int uavqp_swarm_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                          const double* d_times, const double* d_coeff, const int32_t* d_status, int n_groups,
                                          const int32_t* d_group_offsets, const double* d_start, const uavqp_swarm_params* params,
                                          double* d_penalty, double* d_grad_coeff, double* d_grad_times, double* d_grad_start,
                                          double* d_min_sep) {
    const SolvedBatch B{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status};
    bool run;
    const SolvedGroups G{n_groups, d_group_offsets};
    const int rc = solved_args_check(ctx, B, [&] { return swarm_params_valid(params); },
                                     d_penalty || d_grad_coeff || d_grad_times || d_grad_start || d_min_sep, &run, &G);
    if (!run) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return swarm_penalty_enqueue(ctx, B, n_groups, d_group_offsets, d_start, *params, d_penalty, d_grad_coeff, d_grad_times, d_grad_start,
                                 d_min_sep);
}

extern "C" int uavqp_swarm_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                                        const double* coeff, const int32_t* status, int n_groups, const int32_t* group_offsets,
                                        const double* start, const uavqp_swarm_params* params, double* penalty, double* grad_coeff,
                                        double* grad_times, double* grad_start, double* min_sep) {
    const SolvedBatch B{r, n_traj, uniform_segments, seg_offsets, times, coeff, status};
    bool run;
    const SolvedGroups G{n_groups, group_offsets};
    int rc = solved_args_check(ctx, B, [&] { return swarm_params_valid(params); },
                               penalty || grad_coeff || grad_times || grad_start || min_sep, &run, &G);
    if (!run) return rc;
    BatchShape sh;
    rc = swarm_groups_host_check(n_traj, n_groups, group_offsets);
    if (rc == UAVQP_OK) rc = solved_shape(B, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg, ng = (size_t)n_groups;
    Stage st;
    SolvedStage in;
    in.declare(st, B, sh);
    const int i_go = group_offsets ? st.in(group_offsets, sizeof(int32_t) * (ng + 1)) : -1;
    const int i_s = start ? st.in(start, sizeof(double) * n) : -1;
    const int i_p = penalty ? st.out(penalty, sizeof(double) * ng) : -1;
    const int i_g = grad_coeff ? st.out(grad_coeff, sizeof(double) * 3 * 2 * r * tot) : -1;
    const int i_gt = grad_times ? st.out(grad_times, sizeof(double) * tot) : -1;
    const int i_gs = grad_start ? st.out(grad_start, sizeof(double) * n) : -1;
    const int i_ms = min_sep ? st.out(min_sep, sizeof(double) * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = swarm_penalty_enqueue(ctx, in.device(st), n_groups, st.at<int32_t>(i_go), st.at<double>(i_s), *params, st.at<double>(i_p),
                               st.at<double>(i_g), st.at<double>(i_gt), st.at<double>(i_gs), st.at<double>(i_ms));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_swarm_penalty_host");
}
