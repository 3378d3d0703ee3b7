// uavqp_time_opt.h -- host side of uavqp_cost_time_gradient_device / uavqp_time_optimize_device / _host (include/uavqp.h): included by
// uavqp.hip behind the entry points it sequences.  Kernels: qp_time_opt.h (translation unit k_timeopt.hip).
//
// The optimiser is host-side C++ sequencing like the corridor pipeline, but with NO data-dependent control flow on the host: the number of
// launches is fixed by max_iters, every accept / reject is taken per trajectory on the device, and nothing is read back inside the loop:
//     clamp -> solve(times) -> step<INIT> -> max_iters x { solve(trial) -> step<ITER> } -> solve(times)
// The inner solve is uavqp_solve_batch_device itself, so the coefficients handed back are those of a plain solve at the durations handed back.
// With limits (uavqp_time_optimize_limits_device, uavqp_limits.h) every step is preceded by the penalty of the point just solved and the
// backward pass of its coefficient gradient:
//     clamp -> solve(times) -> penalty, backward -> step<INIT> -> max_iters x { solve(trial) -> penalty, backward -> step<ITER> } -> solve(times)
// The order itself is descent_sequence (uavqp_descent.h), here and in every optimiser included behind this file; what they share around it
// is here too: descent_args_check, time_clamp_enqueue and the staging of the _host entries (descent_run_host).
#pragma once
#include "uavqp_descent.h"
static_assert(UAVQP_OK == 0, "descent_sequence goes on while its hooks return 0");

// (uavqp_limits.h, included behind this file and uavqp_adjoint.h)
static int limit_penalty_enqueue(uavqp_ctx* ctx, const SolvedBatch& B, const uavqp_limit_params& L, double* d_penalty, double* d_grad_coeff,
                                 double* d_grad_times, double* d_peak);

extern "C" void uavqp_default_time_opt_params(uavqp_time_opt_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(uavqp_time_opt_params);
    p->max_iters = 24;        // measured: within 2 % of L-BFGS-B's decrease after 10 trials, within 1 % after 20
    p->time_weight = 50.0;
    p->t_min = 1e-2;
    p->t_max = 1e2;
    p->initial_step = 0.1;    // the first trial moves the most sensitive duration by 10 %
    p->armijo_c = 1e-4;
    p->shrink = 0.5;
    p->grow = 2.0;
}

static int topt_grid(const uavqp_ctx* ctx, int n_traj) {
    long long g = ((long long)n_traj * uavqp::TOPT_LPT + 63) / 64;
    if (g > (long long)ctx->num_cus * 32) g = (long long)ctx->num_cus * 32;
    return (int)g;
}

extern "C" int uavqp_cost_time_gradient_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                               const double* d_times, const double* d_coeff, double* d_cost, double* d_grad) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0 || (!d_cost && !d_grad)) return UAVQP_OK;
    if (!d_times || !d_coeff || (uniform_segments == 0 && !d_seg_offsets)) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    uavqp::CostGradArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.seg_offsets = d_seg_offsets; a.times = d_times; a.coeff = d_coeff;
    a.cost = d_cost; a.grad = d_grad;
    const int grid = topt_grid(ctx, n_traj);
    if (r == 3)
        hipLaunchKernelGGL(uavqp::cost_grad_kernel<3>, dim3(grid), dim3(64), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::cost_grad_kernel<4>, dim3(grid), dim3(64), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

static bool topt_params_valid(const uavqp_time_opt_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_time_opt_params)) return false;
    if (p->max_iters < 0 || p->max_iters > 100000) return false;
    if (!(p->time_weight > 0.0 && p->time_weight < INFINITY)) return false;
    if (!(p->t_min > 0.0) || !(p->t_min <= p->t_max) || !(p->t_max < INFINITY)) return false;
    if (!(p->initial_step > 0.0 && p->initial_step < INFINITY)) return false;
    if (!(p->armijo_c > 0.0 && p->armijo_c < 1.0)) return false;
    if (!(p->shrink > 0.0 && p->shrink < 1.0)) return false;
    if (!(p->grow >= 1.0 && p->grow < INFINITY)) return false;
    return true;
}

// What every descent entry refuses, in the precedence their contracts state: ctx, r and the counts (n_groups: the swarm entry's, 1
// elsewhere); the entry's parameter structs (params_ok, called only behind the former); nothing to do -- UAVQP_OK, *run stays false;
// a missing array (arrays: the entry's own pointers, all non-null), offsets or max_segments; uniform_segments x n_traj against
// total_segments; and, under int_rows, the waypoint rows total_segments + n_traj that the kernels count in ints.  *run: the device is set.
template <class ParamsOk>
static int descent_args_check(const uavqp_ctx* ctx, int r, int n_traj, int n_groups, int uniform_segments, int max_segments, int total_segments,
                              const int32_t* d_seg_offsets, bool arrays, bool int_rows, ParamsOk&& params_ok, bool* run) {
    *run = false;
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || n_groups < 0 || uniform_segments < 0 || total_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (!params_ok()) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0 || n_groups == 0) return UAVQP_OK;
    if (!arrays) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && (!d_seg_offsets || max_segments < 1)) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments > 0 && (long long)total_segments != (long long)uniform_segments * n_traj) return UAVQP_ERR_INVALID_ARG;
    if (int_rows && (long long)total_segments > 0x7fffffffLL - n_traj) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    *run = true;
    return UAVQP_OK;
}

// the clamp of the duration optimiser: it reads the span, the durations and the two bounds
static int time_clamp_enqueue(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets, double* d_times, double t_min,
                              double t_max) {
    uavqp::TimeOptArgs k;
    std::memset(&k, 0, sizeof(k));
    k.n_traj = n_traj; k.uniform = uniform_segments; k.seg_offsets = d_seg_offsets; k.times = d_times; k.t_min = t_min; k.t_max = t_max;
    const int grid = topt_grid(ctx, n_traj);
    if (r == 3) hipLaunchKernelGGL(uavqp::time_opt_clamp_kernel<3>, dim3(grid), dim3(64), 0, ctx->stream, k);
    else hipLaunchKernelGGL(uavqp::time_opt_clamp_kernel<4>, dim3(grid), dim3(64), 0, ctx->stream, k);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

// limits = null: uavqp_time_optimize_device.  Otherwise (validated by the caller) f and its gradient carry the limit penalty.
static int time_optimize_run(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                             const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                             const uavqp_time_opt_params* params, double* d_coeff_out, int32_t* d_status_out, double* d_objective_out,
                             int32_t* d_accepted_out, const uavqp_limit_params* limits, double* d_peak_out) {
    bool run;
    int rc = descent_args_check(ctx, r, n_traj, 1, uniform_segments, max_segments, total_segments, d_seg_offsets,
                                d_waypoints && d_times && d_bc && d_coeff_out && d_objective_out, false,
                                [&] { return topt_params_valid(params); }, &run);
    if (!run) return rc;
    const uavqp_time_opt_params P = *params;
    const size_t n = (size_t)n_traj, tot = (size_t)total_segments;

    Carve c;
    const int i_tr = c.add(sizeof(double) * tot), i_gb = c.add(sizeof(double) * tot), i_fb = c.add(sizeof(double) * n), i_al = c.add(sizeof(double) * n);
    const int i_nd = c.add(sizeof(double) * n), i_ac = c.add(sizeof(int32_t) * n), i_st = c.add(sizeof(int32_t) * n);
    const bool lim = limits != nullptr;
    const int i_lg = c.add(sizeof(double) * 3 * 2 * r * tot, lim), i_le = c.add(sizeof(double) * tot, lim), i_lt = c.add(sizeof(double) * tot, lim);
    const int i_lp = c.add(sizeof(double) * n, lim);
    rc = carve_on(ctx->stream, ctx->topt, c);
    if (rc != UAVQP_OK) return rc;
    int32_t* d_st_loop = c.at<int32_t>(i_st);
    int32_t* d_st_final = d_status_out ? d_status_out : d_st_loop;

    uavqp::TimeOptArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.seg_offsets = d_seg_offsets;
    a.times = d_times; a.trial = c.at<double>(i_tr); a.gbest = c.at<double>(i_gb);
    a.coeff = d_coeff_out;
    a.fbest = c.at<double>(i_fb); a.alpha = c.at<double>(i_al); a.need = c.at<double>(i_nd); a.active = c.at<int32_t>(i_ac);
    a.objective = d_objective_out; a.accepted = d_accepted_out;
    a.w = P.time_weight; a.t_min = P.t_min; a.t_max = P.t_max; a.initial_step = P.initial_step; a.armijo = P.armijo_c;
    a.shrink = P.shrink; a.grow = P.grow;
    a.phi = c.at<double>(i_lp); a.lim_explicit = c.at<double>(i_le); a.lim_through = c.at<double>(i_lt);
    const int grid = topt_grid(ctx, n_traj);
    hipStream_t s = ctx->stream;
    // the durations and the status of a point of the sequence; the step kernel reads the status of the solve before it
    auto times_at = [&](const DescentPoint& p) { return p.at == DescentAt::TRIAL ? a.trial : d_times; };
    auto solve = [&](const DescentPoint& p) -> int {
        a.status = p.caller_status ? d_st_final : d_st_loop;
        return uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, times_at(p), d_bc, d_coeff_out,
                                        const_cast<int32_t*>(a.status));
    };
    // the penalty of the point `coeff` was solved at, its gradient in the coefficients, and that gradient taken through the minimiser
    auto penalty_and_backward = [&](const DescentPoint& p) -> int {
        if (!lim) return UAVQP_OK;
        int e = limit_penalty_enqueue(ctx, SolvedBatch{r, n_traj, uniform_segments, d_seg_offsets, times_at(p), d_coeff_out, a.status}, *limits,
                                      c.at<double>(i_lp), c.at<double>(i_lg), c.at<double>(i_le), nullptr);
        if (e != UAVQP_OK) return e;
        return uavqp_solve_backward_device(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, times_at(p),
                                           d_bc, d_coeff_out, a.status, c.at<double>(i_lg), c.at<double>(i_lt), nullptr, nullptr);
    };
    auto step = [&](bool init, int, bool propose) -> int {
        a.propose = propose ? 1 : 0;
        return dispatch_r_flag(r, init, [&](auto R, auto INIT) {
            constexpr int R_ = decltype(R)::value;
            constexpr bool INIT_ = decltype(INIT)::value;
            if (lim) hipLaunchKernelGGL((uavqp::time_opt_step_kernel<R_, INIT_, true>), dim3(grid), dim3(64), 0, s, a);
            else hipLaunchKernelGGL((uavqp::time_opt_step_kernel<R_, INIT_>), dim3(grid), dim3(64), 0, s, a);
        });
    };
    rc = time_clamp_enqueue(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, P.t_min, P.t_max);
    if (rc != UAVQP_OK) return rc;
    rc = descent_sequence(P.max_iters, solve, penalty_and_backward, step);
    if (rc != UAVQP_OK) return rc;
    if (lim && d_peak_out)   // the sampled peaks of what is handed back
        rc = limit_penalty_enqueue(ctx, SolvedBatch{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff_out, d_st_final}, *limits, nullptr,
                                   nullptr, nullptr, d_peak_out);
    return rc;
}

extern "C" int uavqp_time_optimize_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, int total_segments,
                                          const int32_t* d_seg_offsets, const double* d_waypoints, double* d_times, const double* d_bc,
                                          const uavqp_time_opt_params* params, double* d_coeff_out, int32_t* d_status_out,
                                          double* d_objective_out, int32_t* d_accepted_out) {
    return time_optimize_run(ctx, r, n_traj, uniform_segments, max_segments, total_segments, d_seg_offsets, d_waypoints, d_times, d_bc, params,
                             d_coeff_out, d_status_out, d_objective_out, d_accepted_out, nullptr, nullptr);
}

// The device arrays of a descent optimiser's _host entry, as its device implementation takes them (null: an output the entry does not
// have or the caller does not want; extra: the one diagnostic beyond peak / min_dist / outside).
struct DescentStaged {
    int Mmax, total_segments;
    const int32_t* seg_offsets; double* waypoints; double* times; const double* bc;
    double* coeff; int32_t* status; double* objective; int32_t* accepted;
    double* peak; double* min_dist; int32_t* outside; double* extra;
};

// The _host entries of the per-trajectory optimisers: the checks (params_ok: the entry's parameter structs), the staging of the arrays and
// device(DescentStaged) between stage_begin and stage_end.  waypoints_back / times_back: the same pointer where the entry optimises the
// array (inout), null where it only reads it.  extra_out: extra_per_traj doubles per trajectory.  more(Stage&): what an entry stages
// beyond these arrays, declared behind them; its device(DescentStaged, Stage) then finds them on the Stage.
template <class ParamsOk, class Device, class More>
static int descent_run_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                            const double* waypoints, double* waypoints_back, const double* times, double* times_back, const double* bc,
                            ParamsOk&& params_ok, double* coeff_out, int32_t* status_out, double* objective_out, int32_t* accepted_out,
                            double* peak_out, double* min_dist_out, int32_t* outside_out, double* extra_out, size_t extra_per_traj, const char* who,
                            Device&& device, More&& more) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (!params_ok()) return UAVQP_ERR_INVALID_ARG;
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
    const int i_wp = st.add(waypoints, waypoints_back, sizeof(double) * 3 * (tot + n), false);
    const int i_t = st.add(times, times_back, sizeof(double) * tot, false);
    const int i_bc = st.in(bc, sizeof(double) * n * 2 * (r - 1) * 3);
    const int i_out = st.out(coeff_out, sizeof(double) * 3 * 2 * r * tot, true);
    const int i_st = st.out(status_out, sizeof(int32_t) * n);
    const int i_obj = st.out(objective_out, sizeof(double) * 2 * n), i_acc = st.out(accepted_out, sizeof(int32_t) * n);
    const int i_pk = peak_out ? st.out(peak_out, sizeof(double) * 2 * n) : -1;
    const int i_md = min_dist_out ? st.out(min_dist_out, sizeof(double) * n) : -1;
    const int i_o = outside_out ? st.out(outside_out, sizeof(int32_t) * n) : -1;
    const int i_x = extra_out ? st.out(extra_out, sizeof(double) * extra_per_traj * n) : -1;
    more(st);
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = device(DescentStaged{sh.Mmax, (int)sh.total_seg, st.at<int32_t>(i_off), st.at<double>(i_wp), st.at<double>(i_t), st.at<double>(i_bc),
                              st.at<double>(i_out), st.at<int32_t>(i_st), st.at<double>(i_obj), st.at<int32_t>(i_acc), st.at<double>(i_pk),
                              st.at<double>(i_md), st.at<int32_t>(i_o), st.at<double>(i_x)},
                static_cast<const Stage&>(st));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, who);
}
// (an entry without further arrays)
template <class ParamsOk, class Device>
static int descent_run_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                            const double* waypoints, double* waypoints_back, const double* times, double* times_back, const double* bc,
                            ParamsOk&& params_ok, double* coeff_out, int32_t* status_out, double* objective_out, int32_t* accepted_out,
                            double* peak_out, double* min_dist_out, int32_t* outside_out, double* extra_out, size_t extra_per_traj, const char* who,
                            Device&& device) {
    return descent_run_host(
        ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, waypoints_back, times, times_back, bc, params_ok, coeff_out,
        status_out, objective_out, accepted_out, peak_out, min_dist_out, outside_out, extra_out, extra_per_traj, who,
        [&](const DescentStaged& d, const Stage&) { return device(d); }, [](Stage&) {});
}

static int time_optimize_run_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                  const double* waypoints, double* times, const double* bc, const uavqp_time_opt_params* params,
                                  double* coeff_out, int32_t* status_out, double* objective_out, int32_t* accepted_out,
                                  const uavqp_limit_params* limits, double* peak_out, const char* who) {
    return descent_run_host(
        ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, nullptr, times, times, bc, [&] { return topt_params_valid(params); },
        coeff_out, status_out, objective_out, accepted_out, limits ? peak_out : nullptr, nullptr, nullptr, nullptr, 0, who,
        [&](const DescentStaged& d) {
            return time_optimize_run(ctx, r, n_traj, uniform_segments, d.Mmax, d.total_segments, d.seg_offsets, d.waypoints, d.times, d.bc, params,
                                     d.coeff, d.status, d.objective, d.accepted, limits, d.peak);
        });
}

extern "C" int uavqp_time_optimize_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets,
                                        const double* waypoints, double* times, const double* bc, const uavqp_time_opt_params* params,
                                        double* coeff_out, int32_t* status_out, double* objective_out, int32_t* accepted_out) {
    return time_optimize_run_host(ctx, r, n_traj, uniform_segments, max_segments, seg_offsets, waypoints, times, bc, params, coeff_out, status_out,
                                  objective_out, accepted_out, nullptr, nullptr, "uavqp_time_optimize_host");
}
