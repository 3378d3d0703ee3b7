// uavqp_stage.h -- what every host-pointer entry point of include/uavqp.h shares (included by uavqp.hip behind uavqp_ws.h and
// ensure_mapped): the shape of a batch from its CSR offsets, and the layout of the staging buffer.  An entry point declares each of its
// arrays ONCE (Stage::in / out / inout / scratch), then calls stage_begin, its device implementation and stage_end:
//     uploads, clears -> device entry -> downloads -> one stream synchronisation, all on the ctx's stream.
#pragma once

// Total segment count and longest trajectory of a batch.  Ragged: the offsets start at 0 and never decrease; Mmax is clamped DOWN to a
// positive max_segments (longer trajectories are flagged invalid by the kernels, not refused here).  total_seg + n_traj -- the waypoint
// rows -- must fit an int: the device entries count them in ints.
struct BatchShape {
    long long total_seg;
    int Mmax;
};
static int batch_shape(int n_traj, int uniform_segments, int max_segments, const int32_t* seg_offsets, BatchShape* out) {
    long long total_seg = (long long)uniform_segments * n_traj;
    int Mmax = uniform_segments;
    if (uniform_segments == 0) {
        if (seg_offsets[0] != 0) return UAVQP_ERR_INVALID_ARG;
        for (int b = 0; b < n_traj; ++b) {
            const int M = seg_offsets[b + 1] - seg_offsets[b];
            if (M < 0) return UAVQP_ERR_INVALID_ARG;
            if (M > Mmax) Mmax = M;
        }
        total_seg = seg_offsets[n_traj];
        if (max_segments > 0 && max_segments < Mmax) Mmax = max_segments;
        if (Mmax < 1) Mmax = 1;
    }
    if (total_seg > 0x7fffffffLL - n_traj) return UAVQP_ERR_INVALID_ARG;
    *out = BatchShape{total_seg, Mmax};
    return UAVQP_OK;
}

#ifdef UAVQP_HIP   // (as in uavqp_ws.h: batch_shape and the declarations of a Stage compile without the HIP runtime)
// Completion of the latency paths without a stream synchronisation: a one-thread kernel behind the work stamps the word at the head of
// the mapped page, the host polls it (await_host_word).
static int await_mapped_page(uavqp_ctx* ctx, const char* who) {
    const unsigned int seq = ++ctx->pipe_seq;
    volatile unsigned long long* h_word = (volatile unsigned long long*)ctx->h_axis;
    *h_word = 0ull;
    std::atomic_thread_fence(std::memory_order_release);
    hipLaunchKernelGGL(uavqp::host_word_kernel, dim3(1), dim3(1), 0, ctx->stream, (const int32_t*)nullptr, (volatile unsigned long long*)ctx->d_axis, seq);
    return await_host_word(ctx->stream, h_word, seq, nullptr, who);
}

#endif

// The arrays of one call: where each lies is the carver's business (uavqp_ws.h: declaration order, 256-byte boundaries, handle -1 = an
// array this call does not have = a null pointer); Stage adds what is copied where.  The pointers are good for this call only.
struct Stage {
    struct Slot {
        const void* src;   // copied host -> device before the device entry (null: nothing to upload)
        void* dst;         // copied device -> host behind it (null: the caller does not want it, or device-only scratch)
        size_t bytes;
        bool clear;
    } slot[Carve::CAP];
    Carve lay;    // device view of the buffer
    Carve page;   // mapped route only (else unplaced): host view of the same bytes

    int add(const void* src, void* dst, size_t bytes, bool clear) {
        const int i = lay.add(bytes);   // (-1: over the capacity, stage_begin refuses the call)
        if (i >= 0) slot[i] = Slot{src, dst, bytes, clear};
        return i;
    }
    int in(const void* src, size_t bytes) { return add(src, nullptr, bytes, false); }
    // clear: the kernels leave a failed trajectory unwritten and the buffer is reused -- cleared first, it comes back as zeros, never as
    // another batch's coefficients
    int out(void* dst, size_t bytes, bool clear = false) { return add(nullptr, dst, bytes, clear); }
    int inout(void* both, size_t bytes) { return add(both, both, bytes, false); }
    int scratch(size_t bytes) { return add(nullptr, nullptr, bytes, false); }
    template <class T>
    T* at(int i) const { return lay.at<T>(i); }
};

#ifdef UAVQP_HIP
// mapped: the latency route -- the batch lives in the pinned page that is mapped into the device (behind MAPPED_HEAD: the completion
// word has a FIXED slot no payload ever aliases), an upload is a memcpy into the page and the kernels work over the host link.
static int stage_begin(uavqp_ctx* ctx, Stage& st, bool mapped = false) {
    if (st.lay.overflow()) { g_last_error = "host entry: more staging slots than Carve::CAP"; return UAVQP_ERR_ALLOC; }
    const int rc = mapped ? ensure_mapped(ctx, st.lay.total + MAPPED_HEAD) : carve_on(ctx->stream, ctx->stage, st.lay);
    if (rc != UAVQP_OK) return rc;
    if (mapped) {
        st.lay.place((char*)ctx->d_axis + MAPPED_HEAD);
        st.page = st.lay;
        st.page.place((char*)ctx->h_axis + MAPPED_HEAD);
    }
    for (int i = 0; i < st.lay.n; ++i) {
        const Stage::Slot& q = st.slot[i];
        if (q.bytes == 0) continue;
        if (q.src && mapped) std::memcpy(st.page.at<char>(i), q.src, q.bytes);
        else if (q.src) UAVQP_HIP(hipMemcpyAsync(st.lay.at<char>(i), q.src, q.bytes, hipMemcpyHostToDevice, ctx->stream));
        if (q.clear && mapped) std::memset(st.page.at<char>(i), 0, q.bytes);
        else if (q.clear) UAVQP_HIP(hipMemsetAsync(st.lay.at<char>(i), 0, q.bytes, ctx->stream));
    }
    return UAVQP_OK;
}

static int stage_end(uavqp_ctx* ctx, const Stage& st, const char* who) {
    const bool mapped = st.page.base != nullptr;
    if (mapped) {
        const int rc = await_mapped_page(ctx, who);
        if (rc != UAVQP_OK) return rc;
    }
    for (int i = 0; i < st.lay.n; ++i) {
        const Stage::Slot& q = st.slot[i];
        if (!q.dst || q.bytes == 0) continue;
        if (mapped) std::memcpy(q.dst, st.page.at<char>(i), q.bytes);
        else UAVQP_HIP(hipMemcpyAsync(q.dst, st.lay.at<char>(i), q.bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (!mapped) UAVQP_HIP(hipStreamSynchronize(ctx->stream));
    return UAVQP_OK;
}
#endif
