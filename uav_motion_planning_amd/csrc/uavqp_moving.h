// uavqp_moving.h -- host side of uavqp_moving_penalty_device / _host (include/uavqp.h): included by uavqp.hip behind uavqp_attitude.h.
// Kernel: qp_moving.h (translation unit k_moving.hip).  The penalty is one launch, nothing allocated, nothing read back.
// uavqp_moving_optimize_device (uavqp_spacetime_lbfgs.h) enqueues the accumulating variant through moving_penalty_enqueue and stages the
// obstacle arrays of its _host entry through MovingStage.
#pragma once

extern "C" void uavqp_default_moving_params(uavqp_moving_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_moving_params);
    p->samples_per_seg = 8;   // as uavqp_default_limit_params
    p->d_safe = 1.0;          // as uavqp_default_swarm_params
    p->downwash = 1.0;
    p->weight = 1e3;
}

static bool moving_params_valid(const uavqp_moving_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_moving_params)) return false;
    if (p->samples_per_seg < 1) return false;
    if (!(p->d_safe > 0.0 && p->d_safe < INFINITY)) return false;
    if (!(p->downwash >= 1.0 && p->downwash < INFINITY)) return false;
    if (!(p->weight >= 0.0 && p->weight < INFINITY)) return false;
    return true;
}

// what both kinds of entry refuse before they look at a pointer's contents
static bool moving_obstacles_valid(const uavqp_moving_obstacles* o) {
    if (!o || o->struct_size != (int32_t)sizeof(uavqp_moving_obstacles)) return false;
    if (o->n_obs < 0 || o->uniform_segments < 0 || o->n_sets < 0) return false;
    if (o->n_obs > 0 && (!o->times || !o->coeff || (o->uniform_segments == 0 && !o->seg_offsets))) return false;
    if (o->n_sets != 1 && (!o->set_offsets || !o->traj_set)) return false;
    return true;
}

// no trajectory can have an obstacle: the optimiser skips the launch
static bool moving_nothing_to_avoid(const uavqp_moving_obstacles& o) { return o.n_obs == 0 || o.n_sets == 0; }

// What the _host entries check in the contents the device trusts: the obstacle batch's offsets (its shape comes back in *osh), the set
// offsets, traj_set, the radii.
static int moving_host_check(const uavqp_moving_obstacles& o, int n_traj, BatchShape* osh) {
    *osh = BatchShape{0, 1};
    if (o.n_obs > 0) {
        const int rc = batch_shape(o.n_obs, o.uniform_segments, 0, o.seg_offsets, osh);
        if (rc != UAVQP_OK) return rc;
    }
    if (o.set_offsets) {
        if (o.set_offsets[0] != 0 || o.set_offsets[o.n_sets] != o.n_obs) return UAVQP_ERR_INVALID_ARG;
        for (int k = 0; k < o.n_sets; ++k)
            if (o.set_offsets[k + 1] < o.set_offsets[k]) return UAVQP_ERR_INVALID_ARG;
    }
    if (o.traj_set)
        for (int b = 0; b < n_traj; ++b)
            if (o.traj_set[b] < -1 || o.traj_set[b] >= o.n_sets) return UAVQP_ERR_INVALID_ARG;
    if (o.radius)
        for (int i = 0; i < o.n_obs; ++i)
            if (!(o.radius[i] >= 0.0 && o.radius[i] < INFINITY)) return UAVQP_ERR_INVALID_ARG;
    return UAVQP_OK;
}

// The obstacle arrays of a _host entry on its Stage: declare() before stage_begin, device() behind it gives the struct the device
// entry takes.
struct MovingStage {
    int off, t, c, s, rad, so, ts, st;
    void declare(Stage& stage, const uavqp_moving_obstacles& o, int r, int n_traj, const BatchShape& osh) {
        const size_t no = (size_t)o.n_obs, tot = (size_t)osh.total_seg, n = (size_t)n_traj;
        const bool have = o.n_obs > 0;
        off = (have && o.uniform_segments == 0) ? stage.in(o.seg_offsets, sizeof(int32_t) * (no + 1)) : -1;
        t = have ? stage.in(o.times, sizeof(double) * tot) : -1;
        c = have ? stage.in(o.coeff, sizeof(double) * 3 * 2 * r * tot) : -1;
        s = (have && o.start) ? stage.in(o.start, sizeof(double) * no) : -1;
        rad = (have && o.radius) ? stage.in(o.radius, sizeof(double) * no) : -1;
        so = o.set_offsets ? stage.in(o.set_offsets, sizeof(int32_t) * ((size_t)o.n_sets + 1)) : -1;
        ts = o.traj_set ? stage.in(o.traj_set, sizeof(int32_t) * n) : -1;
        st = o.traj_start ? stage.in(o.traj_start, sizeof(double) * n) : -1;
    }
    uavqp_moving_obstacles device(const Stage& stage, const uavqp_moving_obstacles& o) const {
        uavqp_moving_obstacles d = o;
        d.seg_offsets = stage.at<int32_t>(off); d.times = stage.at<double>(t); d.coeff = stage.at<double>(c);
        d.start = stage.at<double>(s); d.radius = stage.at<double>(rad);
        d.set_offsets = stage.at<int32_t>(so); d.traj_set = stage.at<int32_t>(ts); d.traj_start = stage.at<double>(st);
        return d;
    }
};

// (arguments checked by the callers)  accumulate (uavqp_moving_optimize_device only, not in the C ABI): penalty, grad_coeff and grad_times
// are ADDED to what the arrays hold
static int moving_penalty_enqueue(uavqp_ctx* ctx, const SolvedBatch& B, const uavqp_moving_obstacles& O, const uavqp_moving_params& P,
                                  double* d_penalty, double* d_grad_coeff, double* d_grad_times, double* d_grad_start, double* d_min_gap,
                                  int32_t* d_nearest, bool accumulate = false) {
    uavqp::MovingArgs a;
    solved_fill(a, B);
    a.n_obs = O.n_obs; a.o_uniform = O.uniform_segments; a.n_sets = O.n_sets; a.o_seg_offsets = O.seg_offsets; a.o_times = O.times;
    a.o_coeff = O.coeff; a.o_start = O.start; a.o_radius = O.radius; a.set_offsets = O.set_offsets; a.traj_set = O.traj_set;
    a.traj_start = O.traj_start;
    a.penalty = d_penalty; a.grad_coeff = d_grad_coeff; a.grad_times = d_grad_times; a.grad_start = d_grad_start; a.min_gap = d_min_gap;
    a.nearest = d_nearest;
    a.K = P.samples_per_seg;
    a.al16 = coeff_al16(B.coeff, d_grad_coeff);
    a.d_safe = P.d_safe; a.inv_dw2 = 1.0 / (P.downwash * P.downwash); a.weight = P.weight;
    const int grid = topt_grid(ctx, B.n_traj);
    return dispatch_r_flag(B.r, accumulate, [&](auto R, auto ACC) {
        hipLaunchKernelGGL((uavqp::moving_penalty_kernel<decltype(R)::value, decltype(ACC)::value>), dim3(grid), dim3(64), 0, ctx->stream, a);
    });
}

extern "C" int uavqp_moving_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                           const double* d_times, const double* d_coeff, const int32_t* d_status,
                                           const uavqp_moving_obstacles* obstacles, const uavqp_moving_params* params, double* d_penalty,
                                           double* d_grad_coeff, double* d_grad_times, double* d_grad_start, double* d_min_gap,
                                           int32_t* d_nearest) {
    const SolvedBatch B{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status};
    bool run;
    const int rc = solved_args_check(ctx, B, [&] { return moving_params_valid(params) && moving_obstacles_valid(obstacles); },
                                     d_penalty || d_grad_coeff || d_grad_times || d_grad_start || d_min_gap || d_nearest, &run);
    if (!run) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return moving_penalty_enqueue(ctx, B, *obstacles, *params, d_penalty, d_grad_coeff, d_grad_times, d_grad_start, d_min_gap, d_nearest);
}

extern "C" int uavqp_moving_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets,
                                         const double* times, const double* coeff, const int32_t* status,
                                         const uavqp_moving_obstacles* obstacles, const uavqp_moving_params* params, double* penalty,
                                         double* grad_coeff, double* grad_times, double* grad_start, double* min_gap, int32_t* nearest) {
    const SolvedBatch B{r, n_traj, uniform_segments, seg_offsets, times, coeff, status};
    bool run;
    int rc = solved_args_check(ctx, B, [&] { return moving_params_valid(params) && moving_obstacles_valid(obstacles); },
                               penalty || grad_coeff || grad_times || grad_start || min_gap || nearest, &run);
    if (!run) return rc;
    BatchShape sh, osh;
    rc = solved_shape(B, &sh);
    if (rc == UAVQP_OK) rc = moving_host_check(*obstacles, n_traj, &osh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg;
    Stage st;
    SolvedStage in;
    in.declare(st, B, sh);
    MovingStage ms;
    ms.declare(st, *obstacles, r, n_traj, osh);
    const int i_p = penalty ? st.out(penalty, sizeof(double) * n) : -1;
    const int i_g = grad_coeff ? st.out(grad_coeff, sizeof(double) * 3 * 2 * r * tot) : -1;
    const int i_gt = grad_times ? st.out(grad_times, sizeof(double) * tot) : -1;
    const int i_gs = grad_start ? st.out(grad_start, sizeof(double) * n) : -1;
    const int i_mg = min_gap ? st.out(min_gap, sizeof(double) * n) : -1;
    const int i_nr = nearest ? st.out(nearest, sizeof(int32_t) * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = moving_penalty_enqueue(ctx, in.device(st), ms.device(st, *obstacles), *params, st.at<double>(i_p), st.at<double>(i_g), st.at<double>(i_gt),
                                st.at<double>(i_gs), st.at<double>(i_mg), st.at<int32_t>(i_nr));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_moving_penalty_host");
}
