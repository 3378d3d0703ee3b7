// uavqp_spacetime.h -- host side of uavqp_flight_penalty_device / _host and uavqp_spacetime_optimize_device / _host (include/uavqp.h):
// included by uavqp.hip behind uavqp_limits.h and uavqp_esdf.h (whose parameter checks it shares), uavqp_adjoint.h and
// uavqp_waypoint_opt.h (whose sequencing it joins with that of uavqp_time_opt.h).  Kernels: qp_spacetime.h (translation unit k_spacetime.hip).
//
// Like the two optimisers it joins there is NO data-dependent control flow on the host: the number of launches is fixed by max_iters, every
// accept / reject is taken per trajectory on the device, and nothing is read back:
//     anchor copy -> clamp -> solve(waypoints, times) -> flight penalty -> backward -> step<INIT>
//       -> max_iters x { solve(trial waypoints, trial durations) -> flight penalty -> backward -> step<ITER> }
//       -> solve(waypoints, times) -> flight penalty (peak / min_dist / outside only)
// Four launches per iteration.  The inner solve is uavqp_solve_batch_device itself, so the coefficients handed back are those of a plain
// solve at the point handed back.
#pragma once

extern "C" void uavqp_default_spacetime_params(uavqp_spacetime_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_spacetime_params);
    p->max_iters = 32;             // CPU transcription against L-BFGS-B on the test scenes: DESIGN.md section 5.20
    p->smooth_weight = 1.0;        // the defaults of uavqp_default_waypoint_opt_params and uavqp_default_time_opt_params
    p->time_weight = 50.0;
    p->t_min = 1e-2;
    p->t_max = 1e2;
    p->max_move = 2.0;
    p->initial_step_move = 0.1;    // the first trial moves the most sensitive waypoint component by 10 cm
    p->initial_step_log = 0.1;     // ... and the most sensitive duration by 10 %
    p->armijo_c = 1e-4;
    p->shrink = 0.5;
    p->grow = 2.0;
}

static bool spacetime_params_valid(const uavqp_spacetime_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_spacetime_params)) return false;
    if (p->max_iters < 0 || p->max_iters > 100000) return false;
    if (!(p->smooth_weight >= 0.0 && p->smooth_weight < INFINITY)) return false;
    if (!(p->time_weight > 0.0 && p->time_weight < INFINITY)) return false;
    if (!(p->t_min > 0.0) || !(p->t_min <= p->t_max) || !(p->t_max < INFINITY)) return false;
    if (!(p->max_move > 0.0)) return false;   // (INFINITY: no box)
    if (!(p->initial_step_move > 0.0 && p->initial_step_move < INFINITY)) return false;
    if (!(p->initial_step_log > 0.0 && p->initial_step_log < INFINITY)) return false;
    if (!(p->armijo_c > 0.0 && p->armijo_c < 1.0)) return false;
    if (!(p->shrink > 0.0 && p->shrink < 1.0)) return false;
    if (!(p->grow >= 1.0 && p->grow < INFINITY)) return false;
    return true;
}

// the fields uavqp_spacetime_lbfgs_params and uavqp_swarm_opt_params share with the parameters of the projected-gradient entry, as that
// struct (whose validity rule they follow)
template <class P>
static uavqp_spacetime_params spacetime_part_of(const P& p) {
    uavqp_spacetime_params s;
    std::memset(&s, 0, sizeof(s));
    s.struct_size = (int32_t)sizeof(s);
    s.max_iters = p.max_iters;
    s.smooth_weight = p.smooth_weight; s.time_weight = p.time_weight; s.t_min = p.t_min; s.t_max = p.t_max; s.max_move = p.max_move;
    s.initial_step_move = p.initial_step_move; s.initial_step_log = p.initial_step_log; s.armijo_c = p.armijo_c; s.shrink = p.shrink;
    s.grow = p.grow;
    return s;
}

// what the flight penalty needs of its caller: both parameter structs and a distance field of this ctx that has been updated
static bool flight_params_valid(const uavqp_ctx* ctx, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                                const uavqp_clearance_params* clearance) {
    return limit_params_valid(limits) && esdf_usable(ctx, esdf) && esdf->updated && clearance_params_valid(clearance);
}

// (arguments checked by the callers)
static int flight_penalty_enqueue(uavqp_ctx* ctx, const SolvedBatch& B, const uavqp_esdf* esdf, const uavqp_limit_params& L,
                                  const uavqp_clearance_params& C, double* d_penalty, double* d_grad_coeff, double* d_grad_times, double* d_peak,
                                  double* d_min_dist, int32_t* d_outside) {
    uavqp::FlightArgs a;
    solved_fill(a, B);
    a.penalty = d_penalty; a.grad_coeff = d_grad_coeff; a.grad_times = d_grad_times; a.peak = d_peak; a.min_dist = d_min_dist; a.outside = d_outside;
    a.K_lim = L.samples_per_seg; a.K_clr = C.samples_per_seg;
    a.al16 = coeff_al16(B.coeff, d_grad_coeff);
    a.do_lim = (L.weight_v > 0.0 || L.weight_a > 0.0 || d_peak) ? 1 : 0;
    a.do_clr = (C.weight > 0.0 || d_min_dist || d_outside) ? 1 : 0;
    a.v_max = L.v_max; a.a_max = L.a_max; a.inv_v2 = 1.0 / (L.v_max * L.v_max); a.inv_a2 = 1.0 / (L.a_max * L.a_max);
    a.wv = L.weight_v; a.wa = L.weight_a;
    a.d_safe = C.d_safe; a.inv_safe = 1.0 / C.d_safe; a.weight = C.weight;
    a.map = esdf_view(esdf);
    const int grid = topt_grid(ctx, B.n_traj);
    return dispatch_r(B.r, [&](auto R) {
        hipLaunchKernelGGL(uavqp::flight_penalty_kernel<decltype(R)::value>, dim3(grid), dim3(64), 0, ctx->stream, a);
    });
}

extern "C" int uavqp_flight_penalty_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                           const double* d_times, const double* d_coeff, const int32_t* d_status, const uavqp_esdf* esdf,
                                           const uavqp_limit_params* limits, const uavqp_clearance_params* clearance, double* d_penalty,
                                           double* d_grad_coeff, double* d_grad_times, double* d_peak, double* d_min_dist, int32_t* d_outside) {
    const SolvedBatch B{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status};
    bool run;
    const int rc = solved_args_check(ctx, B, [&] { return flight_params_valid(ctx, esdf, limits, clearance); },
                                     d_penalty || d_grad_coeff || d_grad_times || d_peak || d_min_dist || d_outside, &run);
    if (!run) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return flight_penalty_enqueue(ctx, B, esdf, *limits, *clearance, d_penalty, d_grad_coeff, d_grad_times, d_peak, d_min_dist, d_outside);
}

extern "C" int uavqp_flight_penalty_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                                         const double* coeff, const int32_t* status, const uavqp_esdf* esdf, const uavqp_limit_params* limits,
                                         const uavqp_clearance_params* clearance, double* penalty, double* grad_coeff, double* grad_times,
                                         double* peak, double* min_dist, int32_t* outside) {
    const SolvedBatch B{r, n_traj, uniform_segments, seg_offsets, times, coeff, status};
    bool run;
    int rc = solved_args_check(ctx, B, [&] { return flight_params_valid(ctx, esdf, limits, clearance); },
                               penalty || grad_coeff || grad_times || peak || min_dist || outside, &run);
    if (!run) return rc;
    BatchShape sh;
    rc = solved_shape(B, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg;
    Stage st;
    SolvedStage in;
    in.declare(st, B, sh);
    const int i_p = penalty ? st.out(penalty, sizeof(double) * n) : -1;
    const int i_g = grad_coeff ? st.out(grad_coeff, sizeof(double) * 3 * 2 * r * tot) : -1;
    const int i_gt = grad_times ? st.out(grad_times, sizeof(double) * tot) : -1;
    const int i_pk = peak ? st.out(peak, sizeof(double) * 2 * n) : -1;
    const int i_md = min_dist ? st.out(min_dist, sizeof(double) * n) : -1;
    const int i_o = outside ? st.out(outside, sizeof(int32_t) * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = flight_penalty_enqueue(ctx, in.device(st), esdf, *limits, *clearance, st.at<double>(i_p), st.at<double>(i_g), st.at<double>(i_gt),
                                st.at<double>(i_pk), st.at<double>(i_md), st.at<int32_t>(i_o));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_flight_penalty_host");
}

// The workspace slots the three joint optimisers (this file, uavqp_spacetime_lbfgs.h, uavqp_swarm_opt.h) have in common, declared first;
// the line-search state (per trajectory or per swarm) and the L-BFGS history follow with their owners.
struct JointSlots {
    size_t wp_bytes, t_bytes;
    int wt, an, gp, thp;       // trial / anchor / gradient / through waypoints
    int t0, t1, gt, tht, ex;   // the two trial-duration arrays, df/dT at the best point, dPhi/dT through the minimiser and explicit
    int g, ph, ac, st;         // the coefficient gradient, phi, active, the status of the loop
    void declare(Carve& c, int r, size_t n, size_t tot) {
        wp_bytes = sizeof(double) * 3 * (tot + n); t_bytes = sizeof(double) * tot;
        wt = c.add(wp_bytes); an = c.add(wp_bytes); gp = c.add(wp_bytes); thp = c.add(wp_bytes);
        t0 = c.add(t_bytes); t1 = c.add(t_bytes); gt = c.add(t_bytes); tht = c.add(t_bytes); ex = c.add(t_bytes);
        g = c.add(sizeof(double) * 3 * 2 * r * tot);
        ph = c.add(sizeof(double) * n); ac = c.add(sizeof(int32_t) * n); st = c.add(sizeof(int32_t) * n);
    }
};

// One call of a joint optimiser: the batch and the caller's arrays as the device entry got them, the workspace, where each point of the
// sequence (uavqp_descent.h) lives, and the launches the three entries have in common.  The pointers are good behind carve_on(.., c).
struct JointRun {
    uavqp_ctx* ctx;
    int r, n_traj, uniform_segments, max_segments, total_segments;
    const int32_t* d_seg_offsets; double* d_waypoints; double* d_times; const double* d_bc;
    const uavqp_esdf* esdf; const uavqp_limit_params* limits; const uavqp_clearance_params* clearance;
    double* d_coeff_out; int32_t* d_status_out;
    Carve c;
    JointSlots k;

    template <class T>
    T* at(int i) const { return c.at<T>(i); }
    // start and final: the caller's arrays.  Trial it: the trial waypoints, and of the two trial-duration arrays the one of parity it & 1
    // (the step behind that solve reads it and writes the other)
    double* trial_t(int it) const { return at<double>((it & 1) ? k.t1 : k.t0); }
    const double* wp_at(const DescentPoint& p) const { return p.at == DescentAt::TRIAL ? at<double>(k.wt) : d_waypoints; }
    const double* t_at(const DescentPoint& p) const { return p.at == DescentAt::TRIAL ? trial_t(p.it) : d_times; }
    int32_t* status_at(const DescentPoint& p) const { return p.caller_status && d_status_out ? d_status_out : at<int32_t>(k.st); }
    int32_t* status_final() const { return status_at(DescentPoint{DescentAt::FINAL, -1, true}); }   // (of what is handed back)
    // the solved batch at a point of the sequence, and the one that is handed back, as the penalties take it
    SolvedBatch solved_at(const DescentPoint& p) const { return SolvedBatch{r, n_traj, uniform_segments, d_seg_offsets, t_at(p), d_coeff_out, status_at(p)}; }
    SolvedBatch solved_final() const { return SolvedBatch{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff_out, status_final()}; }

    // the identically named fields of SpacetimeArgs and SwarmOptArgs, the ten scalar parameters included
    template <class Args, class Params>
    void fill(Args& a, const Params& P, double* d_objective_out, int32_t* d_accepted_out) const {
        a.n_traj = n_traj; a.uniform = uniform_segments; a.seg_offsets = d_seg_offsets;
        a.waypoints = d_waypoints; a.wp_trial = at<double>(k.wt); a.anchor = at<double>(k.an); a.gp_best = at<double>(k.gp);
        a.times = d_times; a.gt_best = at<double>(k.gt);
        a.coeff = d_coeff_out; a.status = status_at(DescentPoint{DescentAt::START, -1, P.max_iters == 0});
        a.phi = at<double>(k.ph); a.explicit_t = at<double>(k.ex); a.through_p = at<double>(k.thp); a.through_t = at<double>(k.tht);
        a.active = at<int32_t>(k.ac);
        a.objective = d_objective_out; a.accepted = d_accepted_out;
        a.ws = P.smooth_weight; a.wt = P.time_weight; a.t_min = P.t_min; a.t_max = P.t_max; a.max_move = P.max_move;
        a.step_move = P.initial_step_move; a.step_log = P.initial_step_log; a.armijo = P.armijo_c; a.shrink = P.shrink; a.grow = P.grow;
    }
    // what changes from step to step: the durations the last solve ran at, those of the next trial, and whether there is one
    template <class Args>
    void before_step(Args& a, bool init, int it, bool propose) const {
        a.t_eval = init ? d_times : trial_t(it);
        a.t_next = trial_t(it + 1);
        a.propose = propose ? 1 : 0;
    }

    // the start is the centre of the box; the trial waypoints start as a copy too, so that the rows no step writes (a trajectory without a
    // segment) are the caller's
    int anchor_copies(int max_iters) const {
        UAVQP_HIP(hipMemcpyAsync(at<double>(k.an), d_waypoints, k.wp_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        if (max_iters > 0) UAVQP_HIP(hipMemcpyAsync(at<double>(k.wt), d_waypoints, k.wp_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return UAVQP_OK;
    }
    // the inner solve is uavqp_solve_batch_device itself
    int solve(const DescentPoint& p) const {
        return uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, wp_at(p), t_at(p), d_bc, d_coeff_out,
                                        status_at(p));
    }
    // the penalty of the point `coeff` was solved at and its two partial gradients ...
    int flight_penalty(const DescentPoint& p) const {
        return flight_penalty_enqueue(ctx, solved_at(p), esdf, *limits, *clearance, at<double>(k.ph), at<double>(k.g), at<double>(k.ex), nullptr,
                                      nullptr, nullptr);
    }
    // ... and the coefficient gradient taken through the minimiser to the waypoints and the durations by ONE backward pass
    int backward(const DescentPoint& p) const {
        return uavqp_solve_backward_device(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, wp_at(p), t_at(p), d_bc,
                                           d_coeff_out, status_at(p), at<double>(k.g), at<double>(k.tht), at<double>(k.thp), nullptr);
    }
    // The sequence of all three: `a` is the entry's step arguments, more_penalty(point) what it accumulates on the flight penalty before the
    // backward pass, launch(R, INIT) its step kernel (dispatch_r_flag).
    template <class Args, class Penalty, class Launch>
    int descend(Args& a, int max_iters, Penalty&& more_penalty, Launch&& launch) const {
        return descent_sequence(
            max_iters, [&](const DescentPoint& p) -> int { return solve(p); },
            [&](const DescentPoint& p) -> int {
                int e = flight_penalty(p);
                if (e == UAVQP_OK) e = more_penalty(p);
                return e != UAVQP_OK ? e : backward(p);
            },
            [&](bool init, int it, bool propose) -> int {
                before_step(a, init, it, propose);
                return dispatch_r_flag(r, init, launch);
            });
    }
    // the penalty's diagnostics of what is handed back
    int flight_diagnostics(double* d_peak_out, double* d_min_dist_out, int32_t* d_outside_out) const {
        if (!d_peak_out && !d_min_dist_out && !d_outside_out) return UAVQP_OK;
        return flight_penalty_enqueue(ctx, solved_final(), esdf, *limits, *clearance, nullptr, nullptr, nullptr, d_peak_out, d_min_dist_out,
                                      d_outside_out);
    }
};

extern "C" int uavqp_spacetime_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                               const int32_t* d_seg_offsets, double* d_waypoints, double* d_times, const double* d_bc,
                                               const uavqp_esdf* esdf, const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                               const uavqp_spacetime_params* params, double* d_coeff_out, int32_t* d_status_out,
                                               double* d_objective_out, int32_t* d_accepted_out, double* d_peak_out, double* d_min_dist_out,
                                               int32_t* d_outside_out) {
    bool run;
    int rc = descent_args_check(ctx, r, n_traj, 1, uniform_segments, max_segments, total_segments, d_seg_offsets,
                                d_waypoints && d_times && d_bc && d_coeff_out && d_objective_out, true,
                                [&] { return spacetime_params_valid(params) && flight_params_valid(ctx, esdf, limits, clearance); }, &run);
    if (!run) return rc;
    const uavqp_spacetime_params P = *params;
    const size_t n = (size_t)n_traj;

    JointRun j{ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_times, d_bc, esdf, limits, clearance,
               d_coeff_out, d_status_out};
    j.k.declare(j.c, r, n, (size_t)total_segments);
    const int i_fb = j.c.add(sizeof(double) * n), i_al = j.c.add(sizeof(double) * n), i_nd = j.c.add(sizeof(double) * n);
    const int i_sg = j.c.add(sizeof(double) * 2 * n);
    rc = carve_on(ctx->stream, ctx->topt, j.c);
    if (rc != UAVQP_OK) return rc;

    uavqp::SpacetimeArgs a;
    j.fill(a, P, d_objective_out, d_accepted_out);
    a.fbest = j.at<double>(i_fb); a.alpha = j.at<double>(i_al); a.need = j.at<double>(i_nd); a.sigma = j.at<double>(i_sg);
    const int grid = topt_grid(ctx, n_traj);
    rc = j.anchor_copies(P.max_iters);
    if (rc == UAVQP_OK) rc = time_clamp_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, P.t_min, P.t_max);
    if (rc == UAVQP_OK)
        rc = j.descend(a, P.max_iters, [](const DescentPoint&) { return UAVQP_OK; }, [&](auto R, auto INIT) {
            hipLaunchKernelGGL((uavqp::spacetime_step_kernel<decltype(R)::value, decltype(INIT)::value>), dim3(grid), dim3(64), 0, ctx->stream, a);
        });
    if (rc != UAVQP_OK) return rc;
    return j.flight_diagnostics(d_peak_out, d_min_dist_out, d_outside_out);
}

extern "C" int uavqp_spacetime_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                             double* waypoints, double* times, const double* bc, const uavqp_esdf* esdf,
                                             const uavqp_limit_params* limits, const uavqp_clearance_params* clearance,
                                             const uavqp_spacetime_params* params, double* coeff_out, int32_t* status_out, double* objective_out,
                                             int32_t* accepted_out, double* peak_out, double* min_dist_out, int32_t* outside_out) {
    return descent_run_host(
        ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, waypoints, times, times, bc,
        [&] { return spacetime_params_valid(params) && flight_params_valid(ctx, esdf, limits, clearance); }, coeff_out, status_out, objective_out,
        accepted_out, peak_out, min_dist_out, outside_out, nullptr, 0, "uavqp_spacetime_optimize_host", [&](const DescentStaged& d) {
            return uavqp_spacetime_optimize_device(ctx, r, n_traj, uniform_segments, d.Mmax, d.total_segments, d.seg_offsets, d.waypoints, d.times,
                                                   d.bc, esdf, limits, clearance, params, d.coeff, d.status, d.objective, d.accepted, d.peak,
                                                   d.min_dist, d.outside);
        });
}
