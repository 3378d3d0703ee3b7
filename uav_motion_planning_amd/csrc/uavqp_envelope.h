// uavqp_envelope.h -- host side of uavqp_envelope_device / _host (include/uavqp.h): included by uavqp.hip behind uavqp_attitude.h.
// Kernel: qp_envelope.h (translation unit k_envelope.hip).  One launch, nothing allocated, no workspace, nothing read back.
#pragma once

extern "C" void uavqp_default_envelope_params(uavqp_envelope_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));   // every limit 0: its test is off
    p->struct_size = (int32_t)sizeof(uavqp_envelope_params);
    p->depth = 4;                    // 16 leaves: the outer gap is a few 1e-3 of the range (docs/measurement_log.md)
}

static bool envelope_params_valid(const uavqp_envelope_params* p) {
    if (!p || p->struct_size != (int32_t)sizeof(uavqp_envelope_params)) return false;
    if (p->depth < 0 || p->depth > 8) return false;
    for (double x : {p->v_max, p->a_max, p->j_max, p->f_min, p->f_max, p->tilt_max})
        if (!(x >= 0.0 && x < INFINITY)) return false;
    if (p->f_min > 0.0 && p->f_max > 0.0 && p->f_max < p->f_min) return false;
    if (p->tilt_max != 0.0 && !(p->tilt_max < 1.5707963267948966)) return false;
    return true;
}

// (arguments checked by the callers)
static int envelope_enqueue(uavqp_ctx* ctx, const SolvedBatch& B, const uavqp_envelope_params& P, const double* d_box_lo, const double* d_box_hi,
                            double* d_range, double* d_norm, double* d_peak, int32_t* d_seg_verdict, int32_t* d_verdict) {
    uavqp::EnvelopeArgs a;
    solved_fill(a, B);
    a.box_lo = d_box_lo; a.box_hi = d_box_hi;
    a.range = d_range; a.norm = d_norm; a.peak = d_peak; a.seg_verdict = d_seg_verdict; a.verdict = d_verdict;
    a.depth = P.depth;
    a.v2 = P.v_max * P.v_max; a.a2 = P.a_max * P.a_max; a.j2 = P.j_max * P.j_max;
    a.fmin2 = P.f_min * P.f_min; a.fmax2 = P.f_max * P.f_max;
    const double cs = std::cos(P.tilt_max);
    a.cos2 = cs * cs;
    a.tilt_on = P.tilt_max > 0.0 ? 1 : 0;
    const int grid = topt_grid(ctx, B.n_traj);
    return dispatch_r(B.r, [&](auto R) {
        hipLaunchKernelGGL(uavqp::envelope_kernel<decltype(R)::value>, dim3(grid), dim3(64), 0, ctx->stream, a);
    });
}

extern "C" int uavqp_envelope_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                     const double* d_times, const double* d_coeff, const int32_t* d_status,
                                     const uavqp_envelope_params* params, const double* d_box_lo, const double* d_box_hi, double* d_range,
                                     double* d_norm, double* d_peak, int32_t* d_seg_verdict, int32_t* d_verdict) {
    const SolvedBatch B{r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, d_status};
    bool run;
    const int rc = solved_args_check(ctx, B, [&] { return envelope_params_valid(params) && (d_box_lo == nullptr) == (d_box_hi == nullptr); },
                                     d_range || d_norm || d_peak || d_seg_verdict || d_verdict, &run);
    if (!run) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    return envelope_enqueue(ctx, B, *params, d_box_lo, d_box_hi, d_range, d_norm, d_peak, d_seg_verdict, d_verdict);
}

extern "C" int uavqp_envelope_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* seg_offsets, const double* times,
                                   const double* coeff, const int32_t* status, const uavqp_envelope_params* params, const double* box_lo,
                                   const double* box_hi, double* range, double* norm, double* peak, int32_t* seg_verdict, int32_t* verdict) {
    const SolvedBatch B{r, n_traj, uniform_segments, seg_offsets, times, coeff, status};
    bool run;
    int rc = solved_args_check(ctx, B, [&] { return envelope_params_valid(params) && (box_lo == nullptr) == (box_hi == nullptr); },
                               range || norm || peak || seg_verdict || verdict, &run);
    if (!run) return rc;
    BatchShape sh;
    rc = solved_shape(B, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg;
    Stage st;
    SolvedStage in;
    in.declare(st, B, sh);
    const int i_bl = box_lo ? st.in(box_lo, sizeof(double) * 3 * tot) : -1;
    const int i_bh = box_hi ? st.in(box_hi, sizeof(double) * 3 * tot) : -1;
    const int i_r = range ? st.out(range, sizeof(double) * 48 * tot) : -1;
    const int i_n = norm ? st.out(norm, sizeof(double) * 20 * tot) : -1;
    const int i_p = peak ? st.out(peak, sizeof(double) * 20 * n) : -1;
    const int i_sv = seg_verdict ? st.out(seg_verdict, sizeof(int32_t) * tot) : -1;
    const int i_v = verdict ? st.out(verdict, sizeof(int32_t) * n) : -1;
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = envelope_enqueue(ctx, in.device(st), *params, st.at<double>(i_bl), st.at<double>(i_bh), st.at<double>(i_r), st.at<double>(i_n),
                          st.at<double>(i_p), st.at<int32_t>(i_sv), st.at<int32_t>(i_v));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_envelope_host");
}
