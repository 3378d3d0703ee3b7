// uavqp.hip -- HIP kernels + C ABI (include/uavqp.h) of the batched min-jerk / min-snap QP back-end.
// gfx950 only.  The product path has no CPU fallback: every entry point fails with a negative code
// when no device is usable.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/uavqp.h"
#include "qp_device.h"
#include "uavqp_comm.h"

#include "qp_core_kernels.h"
#include "qp_samplers.h"


#include "qp_twisted.h"
#include "qp_generic2.h"
#include "qp_corridor.h"
#include "qp_corridor_dual.h"
#include "qp_rows.h"
#include "qp_rows2.h"
#include "qp_rows_dual.h"
#include "obstacle_grid.h"
#include "qp_time_opt.h"
#include "qp_adjoint.h"
#include "qp_limits.h"
#include "qp_esdf.h"
#include "qp_waypoint_opt.h"
#include "qp_spacetime.h"
#include "qp_spacetime_lbfgs.h"
#include "qp_swarm.h"
#include "qp_swarm_opt.h"
#include "qp_attitude.h"
#include "qp_moving.h"
#include "qp_envelope.h"
#include "qp_clearance_cert.h"
#include "qp_separation_cert.h"
#include "qp_moving_cert.h"
// Measured-slower alternatives kept as bit-identical cross-checks: `make experiments` (-DUAVQP_EXPERIMENTS) only
#ifdef UAVQP_EXPERIMENTS
#include "cloud_grid2d.h"
#include "qp_corridor_lane.h"
#endif

// the solver families are compiled as their own translation units (k_*.hip): here their instantiations are only DECLARED
// (-DUAVQP_SINGLE_TU: a build that includes this file whole -- tools/ubench/twisted_phases.hip -- instantiates everything itself; the
//  lists are read in either build: find_twisted_group goes by them)
#include "kernel_instances.h"
#ifndef UAVQP_SINGLE_TU
UAVQP_INSTANCES_TWISTED3
UAVQP_INSTANCES_TWISTED4
UAVQP_INSTANCES_TWISTED3_ONE
UAVQP_INSTANCES_TWISTED4_ONE
UAVQP_INSTANCES_TWISTED3_GROUP
UAVQP_INSTANCES_TWISTED4_GROUP
UAVQP_INSTANCES_TWISTED3_GROUP8
UAVQP_INSTANCES_TWISTED4_GROUP8
UAVQP_INSTANCES_GENERIC
UAVQP_INSTANCES_CORRIDOR
UAVQP_INSTANCES_CORRIDOR_DUAL
UAVQP_INSTANCES_ROWS31
UAVQP_INSTANCES_ROWS32
UAVQP_INSTANCES_ROWS41
UAVQP_INSTANCES_ROWS42
UAVQP_INSTANCES_ROWS_DUAL
UAVQP_INSTANCES_CLOUD
UAVQP_INSTANCES_TIMEOPT
UAVQP_INSTANCES_ADJOINT
UAVQP_INSTANCES_LIMITS
UAVQP_INSTANCES_ESDF
UAVQP_INSTANCES_WPOPT
UAVQP_INSTANCES_SPACETIME
UAVQP_INSTANCES_SPACETIME_LBFGS
UAVQP_INSTANCES_SWARM
UAVQP_INSTANCES_SWARM_OPT
UAVQP_INSTANCES_ATTITUDE
UAVQP_INSTANCES_MOVING
UAVQP_INSTANCES_ENVELOPE
UAVQP_INSTANCES_CLEARANCE_CERT
UAVQP_INSTANCES_SEPARATION_CERT
UAVQP_INSTANCES_MOVING_CERT
#endif

namespace uavqp {
// Specialised (R, M) instantiations of the register-resident kernel; everything else takes the generic one.
typedef void (*twisted_fn)(UAVQP_TWISTED_SIG);
// The ONE place where a BatchArgs becomes the flat argument list of solve_twisted_kernel (qp_twisted.h), in the kernel's order: the eager
// launch and the rebuilt graph node both pass `ptr` (the runtime copies the values at the call).
struct TwistedParams {
    const double* waypoints;
    const double* times;
    const double* bc;
    double* coeff;
    int32_t* status;
    int n_traj;
#ifdef UAVQP_PHASE_TIMING
    long long* stamps;
    void* ptr[7];
#else
    void* ptr[6];
#endif
    explicit TwistedParams(const BatchArgs& a) : waypoints(a.waypoints), times(a.times), bc(a.bc), coeff(a.coeff), status(a.status), n_traj(a.n_traj) {
        ptr[0] = &waypoints; ptr[1] = &times; ptr[2] = &bc; ptr[3] = &coeff; ptr[4] = &status; ptr[5] = &n_traj;
#ifdef UAVQP_PHASE_TIMING
        stamps = a.stamps;
        ptr[6] = &stamps;
#endif
    }
    TwistedParams(const TwistedParams&) = delete;   // (ptr points into the object itself)
    TwistedParams& operator=(const TwistedParams&) = delete;
};
template <int R, int M>
static twisted_fn twisted_ptr(int tile, bool one) {
    // one: exactly one whole tile per wave -- the instantiation without the tile loop (latency shapes only)
    if (one && tile == 4) return &solve_twisted_kernel<R, M, 4, 16, true>;
    if (one && tile == 8) return &solve_twisted_kernel<R, M, 8, 8, true>;
    if (tile == 4) return &solve_twisted_kernel<R, M, 4, 16>;  // two lane pairs per axis: emission split in two (smallest batches)
    if (tile == 8) return &solve_twisted_kernel<R, M, 8, 8>;  // one lane pair per axis (latency shape)
    return tile == 16 ? &solve_twisted_kernel<R, M, 16> : &solve_twisted_kernel<R, M, 32>;
}
static twisted_fn find_twisted(int r, int M, int tile, bool one) {
#define UAVQP_CASE(RR, MM) if (r == RR && M == MM) return twisted_ptr<RR, MM>(tile, one);
    UAVQP_CASE(4, 2) UAVQP_CASE(4, 3) UAVQP_CASE(4, 4) UAVQP_CASE(4, 5) UAVQP_CASE(4, 6) UAVQP_CASE(4, 7)
    UAVQP_CASE(4, 8) UAVQP_CASE(4, 9) UAVQP_CASE(4, 10) UAVQP_CASE(4, 12)
    UAVQP_CASE(3, 2) UAVQP_CASE(3, 3) UAVQP_CASE(3, 4) UAVQP_CASE(3, 5) UAVQP_CASE(3, 6) UAVQP_CASE(3, 7)
    UAVQP_CASE(3, 8) UAVQP_CASE(3, 10) UAVQP_CASE(3, 12) UAVQP_CASE(3, 16)
#undef UAVQP_CASE
    return nullptr;
}
// The group kernel of a launch that takes the one-tile-per-wave instantiation of (r, M) at this tile, or null where the shape has none
// (kernel_instances.h: the lists): what uavqp_capture_end replays several independent solves of one shape with.
static const void* find_twisted_group(int r, int M, int tile) {
#define UAVQP_CASE4(RR, MM) if (tile == 4 && r == RR && M == MM) return (const void*)&solve_twisted_group_kernel<RR, MM, 4, 16>;
#define UAVQP_CASE8(RR, MM) if (tile == 8 && r == RR && M == MM) return (const void*)&solve_twisted_group_kernel<RR, MM, 8, 8>;
    UAVQP_GROUP_PAIRS4_T4(UAVQP_CASE4) UAVQP_GROUP_PAIRS3_T4(UAVQP_CASE4)
    UAVQP_GROUP_PAIRS4_T8(UAVQP_CASE8) UAVQP_GROUP_PAIRS3_T8(UAVQP_CASE8)
#undef UAVQP_CASE4
#undef UAVQP_CASE8
    return nullptr;
}
// The kernel that replays a group of tile-4 one-tile-per-wave solves of (r, M) with eight trajectories per wave, or null where the shape
// has none (kernel_instances.h: UAVQP_GROUP8_PAIRS*).
static const void* find_twisted_group8(int r, int M) {
#define UAVQP_CASE(RR, MM) if (r == RR && M == MM) return (const void*)&solve_twisted_group8_kernel<RR, MM>;
    UAVQP_GROUP8_PAIRS4(UAVQP_CASE) UAVQP_GROUP8_PAIRS3(UAVQP_CASE)
#undef UAVQP_CASE
    return nullptr;
}
}  // namespace uavqp

namespace uavqp {
// "everything before me on this stream is done": (seq << 32 | *value) into a word of host-coherent pinned memory (value may be null)
// Release side of the hand-over: the system-scope fence BEFORE the store orders everything this stream wrote before the kernel boundary
// (coefficients, statuses: visible to this kernel) ahead of the word; the one behind it pushes the word itself out.
__global__ void host_word_kernel(const int32_t* __restrict__ value, volatile unsigned long long* slot, unsigned int seq) {
    const unsigned int v = value ? (unsigned int)*value : 0u;
    __threadfence_system();
    *slot = ((unsigned long long)seq << 32) | v;
    __threadfence_system();
}
}  // namespace uavqp

// ===================================================================================================
// C ABI
// ===================================================================================================
using uavqp::BatchArgs;

static thread_local std::string g_last_error;

// The host's side of a word the device writes into host-coherent pinned memory (host_word_kernel, compact_order_kernel): poll until its
// upper half is the sequence number awaited.  Bounded: every 65 536 polls the stream is asked -- a failed stream, an idle stream without
// the word, or 60 s without either end the wait.  (Against hipStreamSynchronize / an event: no packet in the stream, and the host
// reacts within the PCIe latency of the store instead of the runtime's wake-up: 17.8 -> 14.6 us for a one-trajectory call.)
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#endif
}
static int await_host_word(hipStream_t s, volatile unsigned long long* w, unsigned int want, unsigned int* value, const char* who) {
    unsigned long long word = *w;
    const auto t_begin = std::chrono::steady_clock::now();
    for (long long spin = 0; (unsigned int)(word >> 32) != want; ++spin) {
        if ((spin & 0xFFFF) == 0xFFFF) {
            const hipError_t q = hipStreamQuery(s);
            const char* what = nullptr;
            if (q != hipSuccess && q != hipErrorNotReady) what = ": the stream failed while a word from the device was awaited";
            else if (q == hipSuccess && (unsigned int)(*w >> 32) != want) what = ": a word from the device never arrived";
            else if (std::chrono::steady_clock::now() - t_begin > std::chrono::seconds(60)) {
                // a long queue in front of the call (a user stream, a very large batch) is not an error: stop polling, wait for the stream the
                // ordinary way -- nothing of this call may still be running against the caller's buffers when the call returns
                const hipError_t e = hipStreamSynchronize(s);
                word = *w;
                if (e == hipSuccess && (unsigned int)(word >> 32) == want) break;
                what = e == hipSuccess ? ": a word from the device never arrived" : ": the stream failed while a word from the device was awaited";
            }
            if (what) {
                (void)hipStreamSynchronize(s);   // (error path: no kernel of this call may outlive it)
                g_last_error = std::string(who) + what;
                return UAVQP_ERR_HIP;
            }
        }
        cpu_relax();
        word = *w;
    }
    std::atomic_thread_fence(std::memory_order_acquire);   // acquire side: the page's payload is read only after the word
    if (value) *value = (unsigned int)(word & 0xFFFFFFFFull);
    return UAVQP_OK;
}

#define UAVQP_HIP(expr)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            g_last_error = std::string(#expr) + ": " + hipGetErrorString(e_);                    \
            return UAVQP_ERR_HIP;                                                                \
        }                                                                                        \
    } while (0)

#include "uavqp_ws.h"
#include "uavqp_capture.h"

// one kernel launch of uavqp_solve_batch_device made while the ctx stream was capturing: what uavqp_capture_end rebuilds the graph from
struct CapturedLaunch {
    const void* fn = nullptr;
    dim3 grid, block;
    unsigned int lds_bytes = 0;
    BatchArgs args{};  // fn != null: a solve_twisted_kernel launch, re-added through TwistedParams (a barrier launch is re-added with the parameters of its captured node)
    const void* group_fn = nullptr;   // the launch took the one-tile-per-wave instantiation and its shape has a group kernel: that kernel
    const void* group8_fn = nullptr;  // ... and the eight-trajectories-per-wave kernel of its shape, where it has one (tile 4 only)
    int tile = 0;                     // trajectories per wave of the launch (fn != null)
};

struct uavqp_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int variant = 0;
    int tile_override = 0;  // fixed tile shape of the specialised kernel (variants 4 / 8 / 16 / 32)
    uavqp_settings settings{};
    int num_cus = 256;
    DevBuf ws;                // scratch of the solvers and the cloud scans: every entry lays it out anew
    uavqp::Comm comm;         // RCCL communicator of the multi-GPU entry points (uavqp_comm_create)
    DevBuf rows_warm2;        // rows part of the starting set of the general-rows solve + the "box phase needed" flags (qp_rows_dual.h)
    void* dbg_queue = nullptr;  // (debug builds) where the last corridor solve kept its work counter
    int dual_trips_extra = 0;   // added to the trip budget 4 n + 16 of the dual preludes (UAVQP_DUAL_TRIPS_EXTRA, may be negative: tools/ experiments)
    int clearance_cert_blocks = 0;   // cap on the blocks of the clearance certificate's launch (UAVQP_CLEARANCE_CERT_BLOCKS; 0: topt_grid's cap
                                     // alone): the tests set it to run the grid-stride loop on a small batch
    int separation_cert_blocks = 0;  // the same for the separation certificate's launch (UAVQP_SEPARATION_CERT_BLOCKS; 0: the cap of its LDS alone)
    int wave_prelude = 2;       // re-solves with G in the cache: 2 = corridor_dual_wave2_kernel (two trajectories per wave), 1 = corridor_dual_wave_kernel (one),
                                // 0 = the batch kernels (UAVQP_WAVE_PRELUDE=0|1|2, UAVQP_NO_WAVE_PRELUDE: A/B runs)
    void* dbg_dual = nullptr;   // (UAVQP_DUAL_DEBUG builds) dump area of corridor_dual_kernel
    void* dbg_guess = nullptr;  // (UAVQP_DUAL_DEBUG builds) the starting sets of the last cold corridor solve
    DevBuf perm;              // ragged dealing permutation (window_sort_kernel); behind it the packed {b, s0, M, 0} records
    DevBuf rows_warm;         // [n_traj][3][2] working set of the box-only phase of uavqp_solve_rows_batch_device
    double* dummy = nullptr;
    int deal_tickets = 1;            // rows_dual_kernel deals its trajectories by ticket (UAVQP_DEAL_TICKETS=0: round-robin as in rounds 4-5, A/B runs)
    // staging buffers of the host-pointer entry points
    DevBuf stage;
    // pinned, device-mapped page of the single-axis entry point (uavqp_solve_axis_host): the kernel reads the inputs of the one
    // trajectory from it and writes coefficients and status into it -- no copy calls on that path
    void* h_axis = nullptr;
    void* d_axis = nullptr;
    size_t axis_bytes = 0;
    // corridor pipeline (uavqp_pipeline.h): device scratch (counters, flags, working sets) and the pinned page its counters are read through
    DevBuf pipe;
    void* h_pipe = nullptr;
    // duration optimiser (uavqp_time_opt.h): trial durations, stored gradient and the per-trajectory state of the descent
    DevBuf topt;
    unsigned int pipe_seq = 0;   // sequence number of the last pipeline round enqueued (uavqp_pipeline.h: tags the count a round reports to the host)
    // between uavqp_capture_begin and uavqp_capture_end: one entry per kernel launch of uavqp_solve_batch_device, in launch order
    bool capturing = false;
    // replay (uavqp_graph_launch): lane 0 of a stage runs on the ctx stream, lane l > 0 on lane_stream[l] (non-blocking, made on first use),
    // forked from the ctx stream by ev_fork and joined to it by ev_join[l]
    hipStream_t lane_stream[uavqp_capture::LANES_MAX] = {};
    hipEvent_t ev_fork = nullptr, ev_join[uavqp_capture::LANES_MAX] = {};
    std::vector<CapturedLaunch> cap_launch;
    std::vector<uavqp_capture::Record> cap_rec;
};

// (capture only) remember a launch just made on the ctx stream; `a` null = a launch that cannot be analysed (a barrier)
static void capture_note(uavqp_ctx* ctx, const void* fn, dim3 grid, dim3 block, size_t lds_bytes, const BatchArgs* a, int r, const void* group_fn = nullptr,
                         const void* group8_fn = nullptr, int tile = 0) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusActive) {   // the capture ended behind the library's back
        ctx->capturing = false;
        ctx->cap_launch.clear();
        ctx->cap_rec.clear();
        return;
    }
    CapturedLaunch l;
    l.fn = fn; l.grid = grid; l.block = block; l.lds_bytes = (unsigned int)lds_bytes;
    l.group_fn = a ? group_fn : nullptr;
    l.group8_fn = a && group_fn ? group8_fn : nullptr;
    l.tile = tile;
    uavqp_capture::Record rec;
    rec.barrier = a == nullptr;
    if (a) {
        l.args = *a;
        const size_t n = (size_t)a->n_traj, tot = n * (size_t)a->uniform;
        rec.read[0] = uavqp_capture::range_of(a->waypoints, sizeof(double) * 3 * (tot + n));
        rec.read[1] = uavqp_capture::range_of(a->times, sizeof(double) * tot);
        rec.read[2] = uavqp_capture::range_of(a->bc, sizeof(double) * n * 2 * (size_t)(r - 1) * 3);
        rec.coeff = uavqp_capture::range_of(a->coeff, sizeof(double) * 3 * 2 * (size_t)r * tot);
        rec.status = uavqp_capture::range_of(a->status, sizeof(int32_t) * n);
    }
    ctx->cap_launch.push_back(l);
    ctx->cap_rec.push_back(rec);
}

#ifndef UAVQP_SRC_HASH
#define UAVQP_SRC_HASH "unknown"
#endif
#ifdef UAVQP_EXPERIMENTS
#define UAVQP_BUILD_TAG ", experiments"
#else
#define UAVQP_BUILD_TAG ""
#endif
extern "C" const char* uavqp_version(void) { return "uavqp 0.6.0 (gfx950, float64, src " UAVQP_SRC_HASH UAVQP_BUILD_TAG ")"; }

extern "C" void uavqp_default_settings(uavqp_settings* out) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = (int32_t)sizeof(uavqp_settings);
    out->warm_start = 1;        // minimum_control.cpp:160
    out->eps_prim_inf = 1e-3;   // minimum_control.cpp:161
    out->max_iter = 0;          // automatic (8 M + 20); the reference's 1000 ADMM iterations (:162) map to an active-set cap
    out->kernel_variant = 0;
    out->ragged_window_sort = 1;
    out->generic_lanes_per_traj = 0;
    out->generic_waves_per_cu = 0;
    out->corridor_pdas_rounds = 3;
    out->corridor_pdas_rounds_warm = 0;
    out->cloud_window = 1;
    out->corridor_tail_shape = 1;
    out->corridor_initial_guess = 2;
    out->rows_lanes_per_problem = 0;
    out->realloc_dead_band = 1.01;
    out->realloc_overshoot = 1.02;
}

static int apply_variant(uavqp_ctx* ctx, int variant);

extern "C" int uavqp_set_settings(uavqp_ctx* ctx, const uavqp_settings* st) {
    if (!ctx || !st || st->struct_size != (int32_t)sizeof(uavqp_settings)) return UAVQP_ERR_INVALID_ARG;
    if (!(st->eps_prim_inf >= 0.0) || !(st->realloc_dead_band >= 1.0) || !(st->realloc_overshoot >= 1.0) || !(st->realloc_dead_band < INFINITY) ||
        !(st->realloc_overshoot < INFINITY) || st->corridor_pdas_rounds < 0 || st->corridor_pdas_rounds > 64 || st->corridor_pdas_rounds_warm < 0 || st->corridor_pdas_rounds_warm > 64 ||
        (st->generic_lanes_per_traj != 0 && st->generic_lanes_per_traj != 1 && st->generic_lanes_per_traj != 2 && st->generic_lanes_per_traj != 3) || st->generic_waves_per_cu < 0 ||
        st->generic_waves_per_cu > 32 || st->rows_lanes_per_problem < 0 || st->rows_lanes_per_problem > 2 ||
        false)
        return UAVQP_ERR_INVALID_ARG;
#ifndef UAVQP_EXPERIMENTS
    // the experimental paths (cloud_window 2 / 3: cloud_grid2d.h; corridor_prelude_lanes 1: qp_corridor_lane.h) exist in `make experiments` builds only
    if (st->cloud_window == 2 || st->cloud_window == 3 || st->corridor_prelude_lanes == 1) {
        g_last_error = "uavqp_set_settings: cloud_window 2 / 3 and corridor_prelude_lanes 1 select experimental kernels; this library was built without -DUAVQP_EXPERIMENTS";
        return UAVQP_ERR_INVALID_ARG;
    }
#endif
    const int rc = apply_variant(ctx, st->kernel_variant);
    if (rc != UAVQP_OK) return rc;
    ctx->settings = *st;
    ctx->settings.warm_start = st->warm_start ? 1 : 0;
    ctx->settings.ragged_window_sort = st->ragged_window_sort == 2 ? 2 : (st->ragged_window_sort ? 1 : 0);     // (2: the dealing as its own launch, rounds 2-5)
    ctx->settings.corridor_initial_guess = st->corridor_initial_guess < 0 ? 0 : (st->corridor_initial_guess > 2 ? 2 : st->corridor_initial_guess);
    // (cloud_window: any value outside 0..3 means "on" = 1, as before round 5; corridor_prelude_lanes sits in what used to be padding: a value
    //  that is none of 0 / 1 / 8 -- a struct filled field by field without uavqp_default_settings -- is taken as the default, not refused)
    ctx->settings.cloud_window = (st->cloud_window >= 0 && st->cloud_window <= 3) ? st->cloud_window : 1;
    ctx->settings.corridor_prelude_lanes = (st->corridor_prelude_lanes == 1 || st->corridor_prelude_lanes == 8) ? st->corridor_prelude_lanes : 0;
    ctx->settings.corridor_tail_shape = st->corridor_tail_shape ? 1 : 0;
    return UAVQP_OK;
}

extern "C" int uavqp_get_settings(const uavqp_ctx* ctx, uavqp_settings* out) {
    if (!ctx || !out) return UAVQP_ERR_INVALID_ARG;
    *out = ctx->settings;
    return UAVQP_OK;
}
extern "C" const char* uavqp_last_error(void) { return g_last_error.c_str(); }

extern "C" int uavqp_create(uavqp_ctx** out_ctx, int device) {
    if (!out_ctx) return UAVQP_ERR_INVALID_ARG;
    *out_ctx = nullptr;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0) {
        g_last_error = "no HIP device visible (the uavqp product path has no CPU fallback)";
        return UAVQP_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n_dev) {
        g_last_error = "device index out of range";
        return UAVQP_ERR_INVALID_ARG;
    }
    UAVQP_HIP(hipSetDevice(device));
    uavqp_ctx* ctx = new (std::nothrow) uavqp_ctx();
    if (!ctx) return UAVQP_ERR_ALLOC;
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cus = prop.multiProcessorCount;
    // A BLOCKING stream: ordered with the legacy default (NULL) stream, which is where a caller that never thinks about
    // streams (and PyTorch by default) fills and reads the buffers it hands over.  Callers that want overlap pass their
    // own stream through uavqp_set_stream.
    e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamDefault);
    if (e != hipSuccess) {
        g_last_error = std::string("hipStreamCreate: ") + hipGetErrorString(e);
        delete ctx;
        return UAVQP_ERR_HIP;
    }
    ctx->stream = ctx->own_stream;
    e = hipMalloc((void**)&ctx->dummy, 4096);
    if (e != hipSuccess) {
        g_last_error = std::string("hipMalloc: ") + hipGetErrorString(e);
        (void)hipStreamDestroy(ctx->own_stream);
        delete ctx;
        return UAVQP_ERR_ALLOC;
    }
    // The environment is read HERE, once, as overrides of the defaults (tuning aids); nothing on the
    // launch path calls getenv.
    uavqp_default_settings(&ctx->settings);
    if (const char* e = std::getenv("UAVQP_TILE")) {
        const int t = std::atoi(e);
        if (t == 4 || t == 8 || t == 16 || t == 32) {
            (void)apply_variant(ctx, t);
            ctx->settings.kernel_variant = t;
        }
    }
    if (std::getenv("UAVQP_NO_LSORT")) ctx->settings.ragged_window_sort = 0;
    if (std::getenv("UAVQP_NO_WAVE_PRELUDE")) ctx->wave_prelude = 0;
    if (const char* e = std::getenv("UAVQP_DEAL_TICKETS")) ctx->deal_tickets = std::atoi(e) != 0;
    if (const char* e = std::getenv("UAVQP_DUAL_TRIPS_EXTRA")) ctx->dual_trips_extra = std::atoi(e);
    if (const char* e = std::getenv("UAVQP_CLEARANCE_CERT_BLOCKS")) { const int v = std::atoi(e); if (v > 0) ctx->clearance_cert_blocks = v; }
    if (const char* e = std::getenv("UAVQP_SEPARATION_CERT_BLOCKS")) { const int v = std::atoi(e); if (v > 0) ctx->separation_cert_blocks = v; }
    if (const char* e = std::getenv("UAVQP_WAVE_PRELUDE")) { const int v = std::atoi(e); if (v >= 0 && v <= 2) ctx->wave_prelude = v; }
    if (const char* e = std::getenv("UAVQP_GENERIC_NAX")) ctx->settings.generic_lanes_per_traj = std::atoi(e) == 3 ? 1 : 3;
    if (const char* e = std::getenv("UAVQP_GENERIC_WPC")) {
        const int w = std::atoi(e);
        if (w > 0 && w <= 32) ctx->settings.generic_waves_per_cu = w;
    }
    *out_ctx = ctx;
    return UAVQP_OK;
}

extern "C" int uavqp_destroy(uavqp_ctx* ctx) {
    if (!ctx) return UAVQP_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm.comm) (void)uavqp_comm_destroy(ctx);
    for (DevBuf* b : {&ctx->ws, &ctx->perm, &ctx->rows_warm, &ctx->rows_warm2, &ctx->stage, &ctx->pipe, &ctx->topt}) dev_free(*b);
    if (ctx->dummy) (void)hipFree(ctx->dummy);
    if (ctx->h_axis) (void)hipHostFree(ctx->h_axis);
    if (ctx->h_pipe) (void)hipHostFree(ctx->h_pipe);
    for (hipStream_t& s : ctx->lane_stream)
        if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (hipEvent_t& e : ctx->ev_join)
        if (e) (void)hipEventDestroy(e);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return UAVQP_OK;
}

extern "C" int uavqp_set_stream(uavqp_ctx* ctx, void* hip_stream) {
    if (!ctx) return UAVQP_ERR_INVALID_ARG;
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return UAVQP_OK;
}

extern "C" int uavqp_synchronize(uavqp_ctx* ctx) {
    if (!ctx) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipStreamSynchronize(ctx->stream));
    return UAVQP_OK;
}

static int apply_variant(uavqp_ctx* ctx, int variant) {
    if (variant == 4 || variant == 8 || variant == 16 || variant == 32) {  // specialised kernel with a fixed tile shape
        ctx->variant = 2;
        ctx->tile_override = variant;
        return UAVQP_OK;
    }
    if (variant < 0 || variant > 2) return UAVQP_ERR_INVALID_ARG;
    ctx->variant = variant;
    ctx->tile_override = 0;
    return UAVQP_OK;
}

extern "C" int uavqp_set_variant(uavqp_ctx* ctx, int variant) {
    if (!ctx) return UAVQP_ERR_INVALID_ARG;
    const int rc = apply_variant(ctx, variant);
    if (rc == UAVQP_OK) ctx->settings.kernel_variant = variant;
    return rc;
}

extern "C" int uavqp_solve_batch_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                        const int32_t* d_seg_offsets, const double* d_waypoints,
                                        const double* d_times, const double* d_bc, double* d_coeff_out,
                                        int32_t* d_status_out) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!d_waypoints || !d_times || !d_bc || !d_coeff_out) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && (!d_seg_offsets || max_segments < 1)) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const int Mmax = uniform_segments > 0 ? uniform_segments : max_segments;

    BatchArgs a;
    a.n_traj = n_traj;
    a.uniform = uniform_segments;
    a.max_segments = Mmax;
    a.seg_offsets = d_seg_offsets;
    a.waypoints = d_waypoints;
    a.times = d_times;
    a.bc = d_bc;
    a.coeff = d_coeff_out;
    a.status = d_status_out;
    a.dummy = ctx->dummy;
    a.fused_sort = 0;
    a.perm = nullptr;
    a.perm4 = nullptr;

    // the specialised kernels move 16 bytes per lane (LDS-DMA loads, dwordx4 stores): every array must be
    // 16-byte aligned (allocations are; a view starting at an odd double is not) -- otherwise the generic
    // kernel, which touches memory 8 bytes at a time, takes the batch
    const bool aligned16 = ((((uintptr_t)d_waypoints) | ((uintptr_t)d_times) | ((uintptr_t)d_bc) | ((uintptr_t)d_coeff_out)) & 15u) == 0;
    if (uniform_segments > 0 && ctx->variant != 1 && aligned16) {
        // Tile shape by batch size (measured on MI355X, 8-segment snap, us per launch over rotating buffers, tools/ubench/tw, round 3 --
        // after the pipelined copy-out of the latency shapes; tiles 4 / 8 / 16 / 32):
        //    1024: 4.00 / 4.44 / 7.4 / -      4096: 5.08 / 5.13 / 8.0 / -     5120: 6.62 / 5.14 / 8.4 / -     8192: 7.38 / 6.02 / 8.8 / -
        //   16384: 11.9 / 9.1 / 10.4 / 10.5   24576: 16.4 / 12.3 / 15.9 / 12.2   32768: - / 16.2 / 16.9 / 15.4   65536: - / 34.4 / 31.6 / 25.4
        // One CU moves only ~10 B/clk, so a small batch is spread over all CUs with fewer trajectories per wave (tile 4: 16 lanes per
        // trajectory, every SIMD busy up to 16 trajectories per CU; tile 8: 8 lanes); a large one wants the full-wave shape that does
        // the least redundant work.  Tile 16 no longer wins anywhere (it stays selectable through uavqp_set_variant).
        // 2026-10-18, with the one-tile-per-wave instantiations, tiles 4 / 8, us per step (bench.py, medians of three runs): replayed graph of 1500
        // steps on two lanes  2048: 2.83 / 2.77   3072: 3.09 / 3.12   4096: 3.38 / 3.31;  of 200 steps  3.08 / 3.07, 3.35 / 3.37, 3.65 / 3.53;  of 20
        // steps (one chain)  5.46 / 5.61, 5.92 / 6.27, 6.08 / 6.35;  eager  5.77 / 5.82, 6.27 / 5.52, 5.73 / 5.88.  Tile 8 is 2-3 % ahead under a
        // two-lane replay at 4096 and 3-6 % behind in the chain of 20 and isolated: the threshold stays.
        int tile = (n_traj <= 16 * ctx->num_cus) ? 4 :((n_traj <= 96 * ctx->num_cus) ? 8 : 32);
        if (ctx->tile_override) tile = ctx->tile_override;
        const int n_tiles = (n_traj + tile - 1) / tile;
        const int max_wg = ctx->num_cus * 4;  // 1 wave / SIMD (register-resident state), persistent over tiles
        const int g = n_tiles < max_wg ? n_tiles : max_wg;
        // One whole tile per wave (whole tiles only, no more tiles than waves): the instantiation without the shifted and the guarded
        // tile, the prefetch and the second input buffer (4096 x 8-segment snap: traced kernel 5.24 -> 4.60 us, replayed step 3.60 -> 3.39).  A function of n_traj and the CU count alone, like the tile: eager and captured
        // launches choose the same kernel.
        const bool one = g == n_tiles && n_traj % tile == 0;
        uavqp::twisted_fn fn = uavqp::find_twisted(r, uniform_segments, tile, one);
        if (fn) {
            a.ws = nullptr;
            uavqp::TwistedParams tp(a);
            UAVQP_HIP(hipLaunchKernel((const void*)fn, dim3(g), dim3(64), tp.ptr, 0, ctx->stream));
            if (ctx->capturing)   // no workspace of the ctx: the one analysable launch
                capture_note(ctx, (const void*)fn, dim3(g), dim3(64), 0, &a, r, one ? uavqp::find_twisted_group(r, uniform_segments, tile) : nullptr,
                             one && tile == 4 ? uavqp::find_twisted_group8(r, uniform_segments) : nullptr, tile);
            return UAVQP_OK;
        }
        if (ctx->variant == 2) {
            g_last_error = "variant 2 requested but no specialised kernel for this (r, segments)";
            return UAVQP_ERR_INVALID_ARG;
        }
    }
    // ragged batches of some size: 256-thread workgroups that deal their chunk to the lanes by segment count
    // Lanes: one per (trajectory, axis) for small batches -- 21 trajectories per wave, a shorter dependent chain per lane
    // (measured, r = 4: M = 14 24 -> 18 us, M = 24 40 -> 29 us up to 4096 trajectories) -- and one per trajectory (3 axes
    // share the factorisation, a third of the E traffic) once the batch is throughput-bound (cross-over at ~8192;
    // 32768 x M = 14: 50 vs 76 us).  Ragged batches of some size deal windows of 16 waves' trajectories by segment count.
    const bool lsort = uniform_segments == 0 && n_traj >= 2048 && ctx->settings.ragged_window_sort;
    int nax = n_traj <= 32 * ctx->num_cus ? 1 : 3;
    if (ctx->settings.generic_lanes_per_traj == 1) nax = 3;       // one lane per trajectory carries all three axes
    else if (ctx->settings.generic_lanes_per_traj == 3) nax = 1;  // one lane per (trajectory, axis)
    // two lanes per trajectory (qp_generic2.h: twisted elimination with a runtime segment count): half the dependent chain
    // per lane and twice the waves
    // (inputs staged in LDS: 32 (4 Mmax + 3) doubles per wave, within the 64 KiB a workgroup gets without opting in)
    const size_t pair_lds = uavqp::generic2_lds_bytes(Mmax);
    // Measured (MI355X, us per launch, lanes per trajectory 1 / 2 / 3-axis-lanes): 32768 ragged M in [4, 24], r = 4: 86 / 54 / 125;
    // r = 3: 72 / 48 / 85; 4096 ragged: 45 / 30 / 36; 1000 ragged: 43 / 26 / 29; 32768 x M = 14: 50 / 41 / 76; x M = 24: 123 / 73 /
    // 178; 262144 x M = 14: 501 / 356 / 716; 32768 x M = 1: 5.4 / 8.5 / 5.9, M = 2: 9.6 / 9.3 / 10.9, M = 3: 13.1 / 13.1 / 15.4
    // (tools/generic2_probe.py) -- the pair kernel everywhere but for the shortest trajectories.
    const bool pair = pair_lds <= 64 * 1024 && aligned16 &&
                      (ctx->settings.generic_lanes_per_traj == 2 || (ctx->settings.generic_lanes_per_traj == 0 && Mmax >= 3));
    if (pair) nax = 3;
    const int ipw = pair ? 32 : (nax == 3 ? 64 : 21);
    const int block = 64;
    int grid = (n_traj + ipw - 1) / ipw;
    // Resident waves: the kernel is bound by the E/h workspace round trip, and the workspace is per resident lane.  With
    // one wave per CU it is ~30 MB (r = 4, M = 14) and stays in L2 while the grid strides over the batch (measured with
    // tools/generic_grid_probe.py: 65536 x M=14: 111 us at 1 wave/CU vs 141 us at 8; 262144: 524 vs 640 us; r = 3, M = 20,
    // 262144: 625 vs 920 us); up to 128 trajectories per CU two waves per CU run the batch in a single round (49 vs 58 us).
    int waves_per_cu = pair ? (int)std::min<size_t>(4, (160 * 1024) / pair_lds) : (nax == 3 ? (n_traj <= 128 * ctx->num_cus ? 2 : 1) : 12);
    if (ctx->settings.generic_waves_per_cu > 0) waves_per_cu = ctx->settings.generic_waves_per_cu;
    const int max_grid = ctx->num_cus * waves_per_cu;
    if (grid > max_grid) grid = max_grid;
    if (lsort) grid = (grid + 15) / 16 * 16;
    const int F = (r - 1) * (r - 1) + nax * (r - 1);
    const size_t ws_bytes = sizeof(double) * (size_t)(Mmax > 1 ? Mmax - 1 : 1) * F * (size_t)grid * block;
    int rc = dev_grow(ctx->stream, ctx->ws, ws_bytes);
    if (rc != UAVQP_OK) return rc;
    a.ws = (double*)ctx->ws.p;
    a.perm = nullptr;
    a.perm4 = nullptr;
    // round 6: the pair kernel's waves rank their window themselves (qp_generic2.h) -- no window_sort_kernel launch in front of the solve, no
    // permutation in HBM; ragged_window_sort = 2 keeps the separate launch (A/B, cross-check test)
    a.fused_sort = (lsort && pair && Mmax <= 63 && ctx->settings.ragged_window_sort != 2) ? 1 : 0;
    if (lsort && !a.fused_sort) {
        // dealing permutation: one counting sort per window of 16 waves' trajectories (see window_sort_kernel)
        // [n_traj] int32 + (16-byte aligned) [n_traj] int4
        const size_t b_perm = align256(sizeof(int32_t) * (size_t)n_traj);
        rc = dev_grow(ctx->stream, ctx->perm, b_perm + sizeof(int4) * (size_t)n_traj);
        if (rc != UAVQP_OK) return rc;
        int32_t* const perm = (int32_t*)ctx->perm.p;
        int4* perm4 = pair ? (int4*)((char*)ctx->perm.p + b_perm) : nullptr;
        const int win = 16 * ipw;
        const int n_win = (n_traj + win - 1) / win;
        if (pair) hipLaunchKernelGGL((uavqp::window_sort_kernel<512>), dim3(n_win), dim3(256), 0, ctx->stream, d_seg_offsets, n_traj, perm, perm4);
        else if (nax == 3) hipLaunchKernelGGL((uavqp::window_sort_kernel<1024>), dim3(n_win), dim3(256), 0, ctx->stream, d_seg_offsets, n_traj, perm, perm4);
        else hipLaunchKernelGGL((uavqp::window_sort_kernel<336>), dim3(n_win), dim3(256), 0, ctx->stream, d_seg_offsets, n_traj, perm, perm4);
        if (ctx->capturing) capture_note(ctx, nullptr, dim3(n_win), dim3(256), 0, nullptr, r);
        a.perm = perm;
        a.perm4 = perm4;
    }
#define UAVQP_GENERIC(RR)                                                                                                   \
    do {                                                                                                                    \
        if (pair) {                                                                                                         \
            if (lsort) hipLaunchKernelGGL((uavqp::solve_generic2_kernel<RR, true>), dim3(grid), dim3(block), pair_lds, ctx->stream, a);  \
            else hipLaunchKernelGGL((uavqp::solve_generic2_kernel<RR, false>), dim3(grid), dim3(block), pair_lds, ctx->stream, a);       \
        } else if (nax == 3) {                                                                                              \
            if (lsort) hipLaunchKernelGGL((uavqp::solve_generic_kernel<RR, true, 3>), dim3(grid), dim3(block), 0, ctx->stream, a);  \
            else hipLaunchKernelGGL((uavqp::solve_generic_kernel<RR, false, 3>), dim3(grid), dim3(block), 0, ctx->stream, a);       \
        } else {                                                                                                            \
            if (lsort) hipLaunchKernelGGL((uavqp::solve_generic_kernel<RR, true, 1>), dim3(grid), dim3(block), 0, ctx->stream, a);  \
            else hipLaunchKernelGGL((uavqp::solve_generic_kernel<RR, false, 1>), dim3(grid), dim3(block), 0, ctx->stream, a);       \
        }                                                                                                                   \
    } while (0)
    if (r == 3) UAVQP_GENERIC(3);
    else UAVQP_GENERIC(4);
#undef UAVQP_GENERIC
    UAVQP_HIP(hipGetLastError());
    if (ctx->capturing) capture_note(ctx, nullptr, dim3(grid), dim3(block), 0, nullptr, r);   // ctx->ws (and ctx->perm): ordered against everything
    return UAVQP_OK;
}

// the pinned, device-mapped staging page of the latency paths (single-axis entry point, small host batches)
static constexpr size_t MAPPED_HEAD = 256;   // head of the mapped page: the completion word of the polled host entries
static int ensure_mapped(uavqp_ctx* ctx, size_t need) {
    if (need <= ctx->axis_bytes) return UAVQP_OK;
    UAVQP_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->h_axis) UAVQP_HIP(hipHostFree(ctx->h_axis));
    ctx->h_axis = ctx->d_axis = nullptr;
    ctx->axis_bytes = 0;
    const size_t cap = need < 65536 ? 65536 : need * 2;
    UAVQP_HIP(hipHostMalloc(&ctx->h_axis, cap, hipHostMallocMapped | hipHostMallocCoherent));
    UAVQP_HIP(hipHostGetDevicePointer(&ctx->d_axis, ctx->h_axis, 0));
    ctx->axis_bytes = cap;
    return UAVQP_OK;
}

#include "uavqp_stage.h"
#include "uavqp_solved.h"

extern "C" int uavqp_solve_batch_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                      const int32_t* seg_offsets, const double* waypoints, const double* times,
                                      const double* bc, double* coeff_out, int32_t* status_out) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!waypoints || !times || !bc || !coeff_out) return UAVQP_ERR_INVALID_ARG;
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
    const int i_out = st.out(coeff_out, sizeof(double) * 3 * 2 * r * tot, true);
    const int i_st = st.out(status_out, sizeof(int32_t) * n);
    // Small batches (a planner's single trajectory, a handful of candidates) are a latency path: the whole batch lives in the
    // pinned page that is mapped into the device, the kernels read and write it over the host link, and the call is the
    // launch(es) plus one polled word instead of 3-4 H2D copies, a memset, 2 D2H copies and a stream synchronisation (measured, one
    // 7-segment trajectory: 72 -> 3x us per call).
    rc = stage_begin(ctx, st, st.lay.total <= 256 * 1024);
    if (rc != UAVQP_OK) return rc;
    rc = uavqp_solve_batch_device(ctx, r, n_traj, uniform_segments, sh.Mmax, st.at<int32_t>(i_off), st.at<double>(i_wp), st.at<double>(i_t),
                                  st.at<double>(i_bc), st.at<double>(i_out), st.at<int32_t>(i_st));
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_solve_batch_host");
}

extern "C" int uavqp_solve_axis_host(uavqp_ctx* ctx, int r, int n_seg, const double* pos_1d, const double* bound_vel,
                                     const double* bound_acc, const double* bound_jerk, const double* time_vec,
                                     double* coef_1d, int32_t* status_out) {
    if (!ctx || (r != 3 && r != 4) || n_seg < 1 || !pos_1d || !bound_vel || !bound_acc || !time_vec || !coef_1d)
        return UAVQP_ERR_INVALID_ARG;
    // One axis of the reference call = a 1-trajectory batch whose other two axes are zero.  The reference's callers solve x, y, z
    // one after the other (test_minimum_jerk.cpp:75,100,125; traj_optimizer.cpp), so this call is a latency path: the batch
    // lives in ONE pinned page that is mapped into the device -- the host writes positions / durations / boundary values
    // there, the kernel reads them over the host link and writes the coefficients and the status next to them, and the call is
    // one kernel launch and one stream synchronisation (the copying entry point underneath it: 3 H2D + memset + 2 D2H).
    const int nd = r - 1, nc = 2 * r;
    const size_t o_wp = 0;
    const size_t o_t = align256(sizeof(double) * 3 * (size_t)(n_seg + 1));
    const size_t o_bc = o_t + align256(sizeof(double) * (size_t)n_seg);
    const size_t o_out = o_bc + align256(sizeof(double) * 2 * 3 * 3);
    const size_t o_st = o_out + align256(sizeof(double) * 3 * (size_t)nc * n_seg);
    const size_t need = o_st + 256 + MAPPED_HEAD;
    UAVQP_HIP(hipSetDevice(ctx->device));
    {
        const int rcm = ensure_mapped(ctx, need);
        if (rcm != UAVQP_OK) return rcm;
    }
    char* hb = (char*)ctx->h_axis + MAPPED_HEAD;   // (completion word: the fixed slot at the head of the page)
    char* db = (char*)ctx->d_axis + MAPPED_HEAD;
    double* wp = (double*)(hb + o_wp);
    for (int i = 0; i <= n_seg; ++i) {
        wp[3 * i] = pos_1d[i];
        wp[3 * i + 1] = 0.0;
        wp[3 * i + 2] = 0.0;
    }
    std::memcpy(hb + o_t, time_vec, sizeof(double) * (size_t)n_seg);
    double* bc = (double*)(hb + o_bc);
    for (int k = 0; k < 2 * 3 * 3; ++k) bc[k] = 0.0;
    for (int e = 0; e < 2; ++e) {
        bc[(e * nd + 0) * 3] = bound_vel[e];
        bc[(e * nd + 1) * 3] = bound_acc[e];
        if (r == 4) bc[(e * nd + 2) * 3] = bound_jerk ? bound_jerk[e] : 0.0;
    }
    volatile int32_t* st = (volatile int32_t*)(hb + o_st);
    *st = 0;
    int rc = uavqp_solve_batch_device(ctx, r, 1, n_seg, n_seg, nullptr, (const double*)(db + o_wp), (const double*)(db + o_t),
                                      (const double*)(db + o_bc), (double*)(db + o_out), (int32_t*)(db + o_st));
    if (rc != UAVQP_OK) return rc;
    rc = await_mapped_page(ctx, "uavqp_solve_axis_host");   // (no stream synchronisation)
    if (rc != UAVQP_OK) return rc;
    const int32_t status = *st;
    if (status == UAVQP_SOLVED) std::memcpy(coef_1d, hb + o_out, sizeof(double) * (size_t)nc * n_seg);   // x axis = the first M rows
    if (status_out) *status_out = status;
    return rc;
}

static void capture_forget(uavqp_ctx* ctx) {
    ctx->capturing = false;
    ctx->cap_launch.clear();
    ctx->cap_rec.clear();
}

extern "C" int uavqp_capture_begin(uavqp_ctx* ctx) {
    if (!ctx) return UAVQP_ERR_INVALID_ARG;
    capture_forget(ctx);
    UAVQP_HIP(hipSetDevice(ctx->device));
    UAVQP_HIP(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    ctx->capturing = true;
    return UAVQP_OK;
}

// The captured chain in launch order, if a chain of kernel nodes is what was captured (one root, every node at most one dependent).
static bool captured_chain(hipGraph_t graph, std::vector<hipGraphNode_t>& order) {
    size_t n = 0, n_root = 0;
    if (hipGraphGetNodes(graph, nullptr, &n) != hipSuccess || n == 0) return false;
    if (hipGraphGetRootNodes(graph, nullptr, &n_root) != hipSuccess || n_root != 1) return false;
    hipGraphNode_t node = nullptr;
    if (hipGraphGetRootNodes(graph, &node, &n_root) != hipSuccess || n_root != 1) return false;
    order.clear();
    while (node) {
        hipGraphNodeType type;
        if (order.size() == n || hipGraphNodeGetType(node, &type) != hipSuccess || type != hipGraphNodeTypeKernel) return false;
        order.push_back(node);
        size_t n_next = 0;
        if (hipGraphNodeGetDependentNodes(node, nullptr, &n_next) != hipSuccess || n_next > 1) return false;
        hipGraphNode_t next = nullptr;
        if (n_next == 1 && (hipGraphNodeGetDependentNodes(node, &next, &n_next) != hipSuccess || n_next != 1)) return false;
        node = next;
    }
    return order.size() == n;
}

// What uavqp_capture_end hands out: the stages of a replay, each a set of chain graphs that run side by side (uavqp_capture.h:
// lay_out).  A capture that is replayed as captured is one stage of one lane.
struct CapturedGraph {
    std::vector<std::vector<hipGraphExec_t>> stage;
    ~CapturedGraph() {
        for (auto& lanes : stage)
            for (hipGraphExec_t e : lanes) (void)hipGraphExecDestroy(e);
    }
};

// The same launches as `captured`, ordered by what they touch instead of by when they were enqueued (uavqp_capture.h): independent solves
// go to different lanes, at most `lanes` of them, and a solve that conflicts with an earlier one follows it in that one's lane.  False when the capture is not exactly the recorded launches of
// uavqp_solve_batch_device, when nothing in it is independent, or when the runtime refuses a step: the caller keeps the captured graph.
// Within a lane, solves of one shape that follow each other and touch disjoint buffers become ONE launch of the group kernel
// (uavqp_capture.h: fuse_groups; qp_twisted.h: solve_twisted_group_kernel) -- also where the replay stays on one lane: up to `fuse` of
// them where that names a count (1..8), and with `fuse` 0 as many as a budget of waves per launch holds in the kernel their group runs:
// `fuse_waves_named` where UAVQP_CAPTURE_FUSE_WAVES names one, else that kernel's own default (uavqp_capture.h: group_cap, fuse_budget, fuse_cap, member_waves).
// (Measured: ONE graph with parallel branches replays slower than the captured chain -- the runtime leaves its single-queue fast path --
//  so every lane of a stage is a chain graph of its own: docs/measurement_log.md.)
static bool rebuild_captured(uavqp_ctx* ctx, hipGraph_t captured, int lanes, int nodes_per_lane, int fuse, int fuse_waves_named, CapturedGraph& out) {
    static_assert(uavqp::GROUP_MAX == uavqp_capture::FUSE_MAX, "a group's pointer sets travel in one kernarg struct");
    const size_t n = ctx->cap_launch.size();
    if (lanes < 1) lanes = 1;
    if ((lanes == 1 && fuse == 1) || n < 2 || n != ctx->cap_rec.size()) return false;
    std::vector<hipGraphNode_t> order;
    if (!captured_chain(captured, order) || order.size() != n) return false;
    std::vector<hipKernelNodeParams> params(n);
    std::vector<uavqp_capture::Shape> shape(n);
    std::vector<int> cap(n, fuse);   // the most members of a group that starts at node k
    for (size_t k = 0; k < n; ++k) {
        const CapturedLaunch& l = ctx->cap_launch[k];
        hipKernelNodeParams& p = params[k];
        if (hipGraphKernelNodeGetParams(order[k], &p) != hipSuccess) return false;
        if ((l.fn && p.func != l.fn) || p.gridDim.x != l.grid.x || p.gridDim.y != l.grid.y || p.gridDim.z != l.grid.z) return false;
        uavqp_capture::Shape& sh = shape[k];
        sh.fn = l.fn; sh.grid = l.grid.x; sh.block = l.block.x; sh.lds_bytes = l.lds_bytes; sh.n_traj = l.args.n_traj;
        sh.one = l.fn && l.group_fn && l.grid.y == 1 && l.grid.z == 1;   // (one kernel function: one group kernel)
        if (fuse < 1) cap[k] = uavqp_capture::group_cap(fuse, fuse_waves_named, l.tile, sh.one, sh.n_traj, sh.grid, l.group8_fn != nullptr);
    }
    if (n > uavqp_capture::NODES_MAX) return false;
    const std::vector<char> status_dead = uavqp_capture::dead_status_stores(ctx->cap_rec);
    const uavqp_capture::Layout lay = uavqp_capture::lay_out(ctx->cap_rec, status_dead, lanes);
    // (The width of a stage goes by its launches in all, not by how they are spread: a stage that is one long chain and a few single
    //  solves pays a fork / join for each of those.  A rotation, what the layout is for, deals its chains evenly.)
    const uavqp_capture::Fused plan = uavqp_capture::fuse_groups(ctx->cap_rec, status_dead, lay, shape, cap, lanes, nodes_per_lane);
    if (!plan.side_by_side && !plan.fused) return false;   // one lane, one launch per solve: the captured chain
    for (size_t s = 0; s < plan.group.size(); ++s) {
        out.stage.emplace_back();
        for (const std::vector<std::vector<int>>& chain : plan.group[s]) {   // one lane of the stage: its groups in capture order, one launch each
            if (chain.empty()) continue;   // the lanes of a stage fill from 0 up: a stage with fewer busy lanes than its width has them in front
            hipGraph_t graph = nullptr;
            if (hipGraphCreate(&graph, 0) != hipSuccess) return false;
            hipGraphNode_t prev = nullptr;
            bool ok = true;
            for (size_t g = 0; ok && g < chain.size(); ++g) {
                const std::vector<int>& members = chain[g];
                const int k = members[0];
                const CapturedLaunch& l = ctx->cap_launch[k];
                BatchArgs a = l.args;
                if (status_dead[k]) a.status = nullptr;        // a later solve overwrites every one of them before anything reads one
                uavqp::TwistedParams tp(a);                    // (every analysable launch is a solve_twisted_kernel: capture_note)
                uavqp::TwistedGroupArgs sets{};
                void* group_ptr[1] = {&sets};
                hipKernelNodeParams p = params[k];             // a barrier: as captured
                if (members.size() > 1) {                      // independent solves of one shape: one launch of the group kernel, grid (n_tiles, members)
                    for (size_t m = 0; m < members.size(); ++m) {
                        const int km = members[m];
                        const BatchArgs& am = ctx->cap_launch[km].args;
                        sets.set[m] = uavqp::TwistedGroupSet{am.waypoints, am.times, am.bc, am.coeff, status_dead[km] ? nullptr : am.status};
                    }
                    // which kernel: uavqp_capture.h: group_kernel_choice (a group of tile-4 launches over a whole number of eights runs eight trajectories per wave)
                    const bool eight = uavqp_capture::group_kernel_choice((int)members.size(), l.tile, shape[k].one, l.args.n_traj, l.group8_fn != nullptr) ==
                                       uavqp_capture::GROUP_EIGHT_PER_WAVE;
                    p = hipKernelNodeParams{};
                    p.func = const_cast<void*>(eight ? l.group8_fn : l.group_fn);
                    p.gridDim = dim3(eight ? (unsigned int)(l.args.n_traj / uavqp::TWMAP8_TILE) : l.grid.x, (unsigned int)members.size());
                    p.blockDim = l.block;
                    p.sharedMemBytes = l.lds_bytes;
                    p.kernelParams = group_ptr;
                } else if (l.fn) {
                    p = hipKernelNodeParams{};
                    p.func = const_cast<void*>(l.fn);
                    p.gridDim = l.grid;
                    p.blockDim = l.block;
                    p.sharedMemBytes = l.lds_bytes;
                    p.kernelParams = tp.ptr;
                }
                hipGraphNode_t node = nullptr;
                ok = hipGraphAddKernelNode(&node, graph, prev ? &prev : nullptr, prev ? 1 : 0, &p) == hipSuccess;   // (the arguments are copied into the node)
                prev = node;
            }
            hipGraphExec_t exec = nullptr;
            ok = ok && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
            (void)hipGraphDestroy(graph);
            if (!ok) return false;
            out.stage.back().push_back(exec);
        }
    }
    // the streams and events the replay forks to and joins through
    if (!ctx->ev_fork && hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess) return false;
    for (int lane = 1; lane < lanes; ++lane) {
        if (!ctx->lane_stream[lane] && hipStreamCreateWithFlags(&ctx->lane_stream[lane], hipStreamNonBlocking) != hipSuccess) return false;
        if (!ctx->ev_join[lane] && hipEventCreateWithFlags(&ctx->ev_join[lane], hipEventDisableTiming) != hipSuccess) return false;
    }
    return true;
}

extern "C" int uavqp_capture_end(uavqp_ctx* ctx, void** out_graph_exec) {
    if (!ctx || !out_graph_exec) return UAVQP_ERR_INVALID_ARG;
    *out_graph_exec = nullptr;
    struct Forget {   // the records of this capture are gone on every way out
        uavqp_ctx* ctx;
        ~Forget() { capture_forget(ctx); }
    } forget{ctx};
    hipGraph_t graph = nullptr;
    UAVQP_HIP(hipStreamEndCapture(ctx->stream, &graph));
    // UAVQP_CAPTURE_LANES = 1..8 (A/B runs; 1 = replay the chain as captured; not set: 2, uavqp_capture.h: REPLAY_LANES_DEFAULT).  GPU_MAX_HW_QUEUES is only read: a process given fewer
    // than 4 hardware queues keeps the chain.  UAVQP_CAPTURE_LANE_NODES: the launches a stage must have per lane (default 16).
    // UAVQP_CAPTURE_FUSE = 1..8: the most independent solves of one shape a launch of the replay carries, for every group (1 = one launch per solve; uavqp_capture.h: fuse_groups).
    // Not set: as many as UAVQP_CAPTURE_FUSE_WAVES (a positive integer, for every kernel; not set: FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT for the eight-per-wave kernel, FUSE_WAVES_DEFAULT for every other) waves per launch hold in the kernel the group runs, 2 to 8 (uavqp_capture.h: group_cap).
    const uavqp_capture::Knobs knobs = uavqp_capture::knobs_from_environment();
    const int lanes = ctx->capturing ? knobs.lanes : 1;
    CapturedGraph* cg = new (std::nothrow) CapturedGraph();
    if (!cg) { (void)hipGraphDestroy(graph); return UAVQP_ERR_ALLOC; }
    if (!rebuild_captured(ctx, graph, lanes, knobs.nodes_per_lane, ctx->capturing ? knobs.fuse_named : 1, knobs.fuse_waves_named, *cg)) {
        (void)hipGetLastError();
        delete cg;
        cg = new (std::nothrow) CapturedGraph();
        if (!cg) { (void)hipGraphDestroy(graph); return UAVQP_ERR_ALLOC; }
        hipGraphExec_t exec = nullptr;
        const hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (e != hipSuccess) {
            (void)hipGraphDestroy(graph);
            delete cg;
            g_last_error = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
            return UAVQP_ERR_HIP;
        }
        cg->stage.emplace_back(1, exec);
    }
    (void)hipGraphDestroy(graph);
    *out_graph_exec = (void*)cg;
    return UAVQP_OK;
}

// Lane 0 of every stage replays on the ctx stream; the other lanes wait for what the ctx stream holds so far (ev_fork) and the ctx stream
// waits for each of them (ev_join) before the next stage, or whatever the caller enqueues behind the replay, starts.
extern "C" int uavqp_graph_launch(uavqp_ctx* ctx, void* graph_exec) {
    if (!ctx || !graph_exec) return UAVQP_ERR_INVALID_ARG;
    const CapturedGraph* cg = (const CapturedGraph*)graph_exec;
    for (const std::vector<hipGraphExec_t>& lanes : cg->stage) {
        const size_t m = lanes.size();
        if (m > 1) UAVQP_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
        for (size_t l = 1; l < m; ++l) {
            UAVQP_HIP(hipStreamWaitEvent(ctx->lane_stream[l], ctx->ev_fork, 0));
            UAVQP_HIP(hipGraphLaunch(lanes[l], ctx->lane_stream[l]));
            UAVQP_HIP(hipEventRecord(ctx->ev_join[l], ctx->lane_stream[l]));
        }
        UAVQP_HIP(hipGraphLaunch(lanes[0], ctx->stream));
        for (size_t l = 1; l < m; ++l) UAVQP_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join[l], 0));
    }
    return UAVQP_OK;
}

extern "C" int uavqp_graph_destroy(uavqp_ctx* ctx, void* graph_exec) {
    if (!ctx) return UAVQP_ERR_INVALID_ARG;
    delete (CapturedGraph*)graph_exec;
    return UAVQP_OK;
}

extern "C" int uavqp_eval_batch_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                       const double* d_times, const double* d_coeff, int n_samples, double t0, double dt,
                                       int what, double* d_out) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || n_samples < 0 || uniform_segments < 0 || (what & 7) == 0)
        return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0 || n_samples == 0) return UAVQP_OK;
    if (!d_times || !d_coeff || !d_out || (uniform_segments == 0 && !d_seg_offsets)) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    uavqp::EvalArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.n_samples = n_samples; a.what = what & 7;
    a.seg_offsets = d_seg_offsets; a.times = d_times; a.coeff = d_coeff; a.t0 = t0; a.dt = dt; a.out = d_out;
    const long long total = (long long)n_traj * n_samples;
    long long grid = (total + 255) / 256;
    const long long cap = (long long)ctx->num_cus * 16;
    if (grid > cap) grid = cap;
    if (r == 3)
        hipLaunchKernelGGL(uavqp::eval_kernel<3>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::eval_kernel<4>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_traj_length_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                        const double* d_times, const double* d_coeff, double dt, double* d_length, double* d_mean_vel,
                                        int32_t* d_n_samples) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || !(dt > 0.0) || !(dt < INFINITY)) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!d_times || !d_coeff || (uniform_segments == 0 && !d_seg_offsets)) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    uavqp::LengthArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.seg_offsets = d_seg_offsets; a.times = d_times; a.coeff = d_coeff; a.dt = dt;
    a.length = d_length; a.mean_vel = d_mean_vel; a.n_samples = d_n_samples;
    int grid = n_traj < ctx->num_cus * 32 ? n_traj : ctx->num_cus * 32;
    if (r == 3)
        hipLaunchKernelGGL(uavqp::traj_length_kernel<3>, dim3(grid), dim3(64), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::traj_length_kernel<4>, dim3(grid), dim3(64), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

// Dealing order of a ragged batch (longest trajectory first; seg_hist / seg_scan / seg_scatter_kernel): order [n_traj], then the histogram
// and the cursors (256 ints each) -- align256(4 n_traj) + 2048 bytes, declared on the caller's layout by length_order_slots (absent:
// nothing is reserved).  The order depends on the segment counts only: a caller that re-solves the same batch (the config-5 pipeline)
// makes it once and passes it to corridor_warm_impl.
struct LengthOrder { int order, hist; };
static LengthOrder length_order_slots(Carve& c, int n_traj, bool present) {
    return LengthOrder{c.add(sizeof(int32_t) * (size_t)n_traj, present), c.add(2048, present)};
}
static int make_length_order(uavqp_ctx* ctx, const int32_t* d_seg_offsets, int n_traj, const Carve& c, LengthOrder lo, const int32_t** d_order_out) {
    int32_t* d_order = c.at<int32_t>(lo.order);
    int* d_hist = c.at<int>(lo.hist);
    int* d_cursor = d_hist + 256;
    UAVQP_HIP(hipMemsetAsync(d_hist, 0, 256 * sizeof(int), ctx->stream));
    int sg = (n_traj + 255) / 256;
    if (sg > ctx->num_cus * 4) sg = ctx->num_cus * 4;
    hipLaunchKernelGGL(uavqp::seg_hist_kernel, dim3(sg), dim3(256), 0, ctx->stream, d_seg_offsets, n_traj, d_hist);
    hipLaunchKernelGGL(uavqp::seg_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, d_hist, d_cursor);
    hipLaunchKernelGGL(uavqp::seg_scatter_kernel, dim3(sg), dim3(256), 0, ctx->stream, d_seg_offsets, n_traj, d_cursor, d_order);
    *d_order_out = d_order;
    return UAVQP_OK;
}

// Waypoint rows of a batch, sum(M_b) + n_traj.  Ragged with total_segments < 0 (unknown): the last CSR offset is only known on the
// device; a 4-byte read-back (synchronous on the ctx stream).
static int batch_rows(uavqp_ctx* ctx, int n_traj, int uniform_segments, long long total_segments, const int32_t* d_seg_offsets, long long* rows) {
    if (uniform_segments > 0) *rows = (long long)n_traj * (uniform_segments + 1);
    else if (total_segments >= 0) *rows = total_segments + n_traj;
    else {
        int32_t last = 0;
        UAVQP_HIP(hipMemcpyAsync(&last, d_seg_offsets + n_traj, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        UAVQP_HIP(hipStreamSynchronize(ctx->stream));
        if (last < 0) return UAVQP_ERR_INVALID_ARG;
        *rows = (long long)last + n_traj;
    }
    return UAVQP_OK;
}

// total_segments < 0: unknown -- for a ragged batch the last CSR offset is then read back from the device (4 bytes, one stream
// synchronisation); callers that know it (the host-pointer entries, the rows solver's second phase, the corridor pipeline) pass it
// and the call stays asynchronous.
static int corridor_warm_impl(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                              const int32_t* d_seg_offsets, const double* d_waypoints, const double* d_times,
                              const double* d_bc, const double* d_corr_lo, const double* d_corr_hi,
                              double* d_coeff_out, int32_t* d_status_out, int32_t* d_iters_out,
                              uint64_t* d_active_set, int warm_start, long long total_segments, const int32_t* d_order_ready = nullptr,
                              const int32_t* d_only_i32 = nullptr, const unsigned char* d_only_u8 = nullptr,
                              double* d_gcache = nullptr, const double* d_gscale = nullptr, int gcache_mode = 0,
                              const int32_t* d_compact_ready = nullptr, const int* d_n_active_ready = nullptr) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!d_waypoints || !d_times || !d_bc || !d_corr_lo || !d_corr_hi || !d_coeff_out || !d_status_out) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && (!d_seg_offsets || max_segments < 1)) return UAVQP_ERR_INVALID_ARG;
    if (warm_start && !d_active_set) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const int Mmax = uniform_segments > 0 ? uniform_segments : max_segments;
    uavqp::CorridorArgs a;
    a.active = (unsigned long long*)d_active_set; a.warm = warm_start == 2 ? 2 : (warm_start ? 1 : 0);
    a.n_traj = n_traj; a.uniform = uniform_segments; a.max_segments = Mmax; a.max_iter = ctx->settings.max_iter > 0 ? ctx->settings.max_iter : 8 * Mmax + 20;
    // cold start: 0 = empty set, 1 = closed-form set of the prep kernel, 2 = the set the position-space dual method ends with
    // (qp_corridor_dual.h; trajectories of up to 33 segments, longer batches fall back to 1) -- then no block-pivot rounds: the set
    // only has to be verified
    const int gmode = warm_start ? 0 : ctx->settings.corridor_initial_guess;
    const bool dual = gmode == 2 && Mmax >= 2 && Mmax - 1 <= 32;
    a.pdas_rounds = warm_start ? ctx->settings.corridor_pdas_rounds_warm : (dual ? 0 : ctx->settings.corridor_pdas_rounds);
    a.guess_closed_form = (gmode != 0 && !dual) ? 1 : 0;
    a.fused_emit = 1;      // the solve kernel writes the polynomials itself (corridor_emit_kernel: only behind the rows solvers)
    a.only_i32 = d_only_i32; a.only_u8 = d_only_u8;
    a.gcache = d_gcache; a.gscale = d_gscale; a.gcache_mode = (d_gcache && Mmax - 1 <= 24) ? gcache_mode : 0;
    a.seg_offsets = d_seg_offsets; a.waypoints = d_waypoints; a.times = d_times; a.bc = d_bc;
    a.corr_lo = d_corr_lo; a.corr_hi = d_corr_hi; a.coeff = d_coeff_out; a.status = d_status_out; a.iters = d_iters_out;
    // Persistent single-wave workgroups, one per SIMD (the sweep state of a lane pair lives in LDS: 4 x 40 KiB per CU),
    // 32 problems in flight per wave, refilled from the work counter.
    const long long pairs = 3LL * n_traj;
    long long grid = (pairs + 31) / 32;
    const int own_max_ = ((uniform_segments > 0 ? uniform_segments : max_segments) + 1) / 2;
    // Small batches of long snap problems are bound by the slowest problem's chain of iterations, not by throughput: two waves per CU
    // with ten instead of five own knots per lane on chip make every iteration of a 24-segment problem ~13 % shorter (config 5: five
    // rounds 5.85 -> 5.64 ms) where four waves per CU would not be kept busy anyway; large batches (config 3) lose 50 % that way.
    const bool tail_shape = r == 4 && UAVQP_CORRIDOR_WAVES_PER_CU == 4 && own_max_ > uavqp::corridor_lds_knots(4) && pairs <= 4LL * ctx->num_cus * 2 * 32 &&
                            ctx->settings.corridor_tail_shape != 0;
    const int wpc = tail_shape ? 2 : uavqp::corridor_waves_per_cu();
    const long long max_grid = (long long)ctx->num_cus * wpc;
    if (grid > max_grid) grid = max_grid;
    const int NT = uavqp::corridor_lds_knots(r, wpc);
    const int F = r * (r + 1) / 2 + r + 1;  // must match corridor_solve_kernel's state layout
    const int own_max = (Mmax + 1) / 2;        // own knots of the longer half, meeting knot included
    const int ws_knots = own_max > NT ? own_max - NT : 0;
    long long rows = 0;                        // waypoint rows of the batch
    int rc = batch_rows(ctx, n_traj, uniform_segments, total_segments, d_seg_offsets, &rows);
    if (rc != UAVQP_OK) return rc;
    // (a caller that hands over a compacted dealing order -- the rows solve's box phase, the pipeline -- has decided the order: no window sort nobody reads)
    const bool deal_by_length = uniform_segments == 0 && n_traj >= 64 && ctx->settings.ragged_window_sort && !d_order_ready && !(d_compact_ready && d_n_active_ready);
    const bool guess = gmode != 0;     // cold start from a starting set (closed form: prep kernel; dual method: corridor_dual_kernel)
    const bool masked = d_only_i32 || d_only_u8;
    Carve c;
    const int i_xsol = c.add(sizeof(double) * 3 * (size_t)r * (size_t)rows);   // (reserved, never touched while fused_emit = 1: DESIGN.md section 1)
    const int i_queue = c.add(256);            // the work counter; debug builds: the stamps at + 64 (UAVQP_CORRIDOR_TIMING)
    const int i_desc = c.add(sizeof(unsigned long long) * 3 * (size_t)n_traj);
    const LengthOrder i_order = length_order_slots(c, n_traj, deal_by_length);
    const int i_state = c.add(sizeof(double) * (size_t)ws_knots * F * (size_t)grid * 64, ws_knots > 0);
    const int i_guess = c.add(sizeof(unsigned long long) * 6 * (size_t)n_traj, guess);
    // compacted dealing order + its length -- reserved whether this solve is masked or not (4 bytes per trajectory): the first masked solve of a
    // pipeline call must not grow the workspace, i.e. stop the stream and re-allocate, in the middle of the loop
    const int i_compact = c.add(sizeof(int32_t) * (size_t)n_traj), i_n_active = c.add(256);
    // one lane per trajectory (qp_corridor_lane.h): batches of at most 16 segments per trajectory, G not cached across solves
#ifdef UAVQP_EXPERIMENTS
    const bool lane_prelude = dual && !(d_gcache && gcache_mode != 0) && Mmax - 1 <= uavqp::LANE_NV && ctx->settings.corridor_prelude_lanes == 1;
    long long lgrid = ((long long)n_traj + 63) / 64;
    if (lgrid > (long long)ctx->num_cus * 4) lgrid = (long long)ctx->num_cus * 4;     // (one wave per SIMD: the register file, not the 27 KB of LDS per wave, sets it)
    const int i_lane = c.add(sizeof(double) * (size_t)uavqp::lane_scratch_doubles(r) * (size_t)lgrid, lane_prelude);
#endif
    rc = carve_on(ctx->stream, ctx->ws, c);
    if (rc != UAVQP_OK) return rc;
    a.guess = c.at<unsigned long long>(i_guess);
    a.coeff = d_coeff_out;
    a.xsol = c.at<double>(i_xsol);
    a.queue = c.at<unsigned int>(i_queue);
    ctx->dbg_queue = a.queue;
    a.desc = c.at<unsigned long long>(i_desc);
    a.ws = c.at<double>(i_state);
    a.ws_knots = ws_knots;
    a.order = d_order_ready;
    if (deal_by_length) {
        rc = make_length_order(ctx, d_seg_offsets, n_traj, c, i_order, &a.order);
        if (rc != UAVQP_OK) return rc;
    }
    a.n_active = nullptr;
    if (masked && d_compact_ready && d_n_active_ready) {
        // (the caller compacted the dealing order of the participating trajectories already: the pipeline does it right behind the
        // re-allocation whose flags are the mask, where the count doubles as "how many did it stretch")
        a.order = d_compact_ready;
        a.n_active = d_n_active_ready;
    } else if (masked) {
        int32_t* d_compact = c.at<int32_t>(i_compact);
        int* d_n_active = c.at<int>(i_n_active);
        hipLaunchKernelGGL(uavqp::compact_order_kernel, dim3(1), dim3(1024), 0, ctx->stream, a.order, n_traj, d_only_i32, d_only_u8, d_compact, d_n_active);
        a.order = d_compact;
        a.n_active = d_n_active;
    }
#ifdef UAVQP_DUAL_DEBUG
    {
        static double* s_dbg = nullptr;
        if (!s_dbg) { UAVQP_HIP(hipMalloc(&s_dbg, 64 * 2048 * sizeof(double))); }
        if (gcache_mode != 2) UAVQP_HIP(hipMemsetAsync(s_dbg, 0, 64 * 2048 * sizeof(double), ctx->stream));   // (re-solves of a pipeline call keep what the wave prelude recorded)
        a.dbg = s_dbg;
        ctx->dbg_dual = s_dbg;
        ctx->dbg_guess = a.guess;
    }
#endif
#ifdef UAVQP_CORRIDOR_TIMING
    a.stamps = (long long*)((char*)a.queue + 64);   // debug build: section cycles of wave 0, read back by uavqp_debug_corridor_stamps
#endif
    if (!dual) UAVQP_HIP(hipMemsetAsync(a.queue, 0, sizeof(unsigned int), ctx->stream));     // (with a prelude: its first block resets the work counter)
    // with the dual prelude in front, resetting, validating and describing the problems is its business (one launch less, and the inputs are
    // not read a third time); otherwise corridor_reset_kernel + corridor_prep_kernel
    a.prep_in_dual = dual ? 1 : 0;
    if (!a.prep_in_dual) {
        hipLaunchKernelGGL(uavqp::corridor_reset_kernel, dim3((n_traj + 255) / 256), dim3(256), 0, ctx->stream, d_status_out, d_iters_out, n_traj, d_only_i32, d_only_u8);
        long long pgrid = (pairs + 255) / 256;
        if (pgrid > (long long)ctx->num_cus * 16) pgrid = (long long)ctx->num_cus * 16;
        if (r == 3) hipLaunchKernelGGL(uavqp::corridor_prep_kernel<3>, dim3((unsigned)pgrid), dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL(uavqp::corridor_prep_kernel<4>, dim3((unsigned)pgrid), dim3(256), 0, ctx->stream, a);
    }
    if (dual && gcache_mode == 2 && d_gcache && d_gscale && ctx->wave_prelude) {
        // G of every trajectory is in the cache of an earlier solve of this outer loop: one trajectory per wave, no chain, no lockstep
        if (ctx->wave_prelude == 2) {   // two trajectories per wave (lanes 0-31 / 32-63)
            long long wgrid = (long long)n_traj < (long long)ctx->num_cus * 8 ? (long long)n_traj : (long long)ctx->num_cus * 8;
            if (wgrid < 1) wgrid = 1;
            if (r == 3) hipLaunchKernelGGL((uavqp::corridor_dual_wave2_kernel<3>), dim3((unsigned)wgrid), dim3(64), 0, ctx->stream, a, ctx->dual_trips_extra);
            else hipLaunchKernelGGL((uavqp::corridor_dual_wave2_kernel<4>), dim3((unsigned)wgrid), dim3(64), 0, ctx->stream, a, ctx->dual_trips_extra);
        } else {
            long long wgrid = (long long)n_traj < (long long)ctx->num_cus * 12 ? (long long)n_traj : (long long)ctx->num_cus * 12;
            if (wgrid < 1) wgrid = 1;
            if (r == 3) hipLaunchKernelGGL((uavqp::corridor_dual_wave_kernel<3>), dim3((unsigned)wgrid), dim3(64), 0, ctx->stream, a, ctx->dual_trips_extra);
            else hipLaunchKernelGGL((uavqp::corridor_dual_wave_kernel<4>), dim3((unsigned)wgrid), dim3(64), 0, ctx->stream, a, ctx->dual_trips_extra);
        }
#ifdef UAVQP_EXPERIMENTS
    } else if (lane_prelude) {
        double* const d_lane = c.at<double>(i_lane);
        if (r == 3) hipLaunchKernelGGL((uavqp::corridor_dual_lane_kernel<3>), dim3((unsigned)lgrid), dim3(64), 0, ctx->stream, a, d_lane, ctx->dual_trips_extra);
        else hipLaunchKernelGGL((uavqp::corridor_dual_lane_kernel<4>), dim3((unsigned)lgrid), dim3(64), 0, ctx->stream, a, d_lane, ctx->dual_trips_extra);
#endif
    } else if (dual) {
        // groups of 8 lanes (two tableau columns each) for the trajectories of up to 17 segments, whole DPP rows for the longer ones: a batch
        // of mixed lengths gets both launches, each skipping (per wave: the dealing order is by length) what the other one takes
        auto launch_dual = [&](int L, int NRW, int n_lo, int last) {
            const long long nb = ((long long)n_traj + 64 / L - 1) / (64 / L);
            const int lds_b = 8 * (64 / L) * uavqp::corridor_dual_lds_doubles(r, L, NRW);
            int wpc_d = (160 * 1024) / lds_b;
            const int wmax = NRW <= 24 ? 8 : 4;                   // (registers: two waves per SIMD up to 24 tableau rows, one beyond)
            if (wpc_d > wmax) wpc_d = wmax;
            if (wpc_d < 1) wpc_d = 1;
            const long long dgrid = nb < (long long)ctx->num_cus * wpc_d ? nb : (long long)ctx->num_cus * wpc_d;
#define UAVQP_DUAL_LAUNCH(R_, L_, N_) hipLaunchKernelGGL((uavqp::corridor_dual_kernel<R_, L_, N_>), dim3((unsigned)dgrid), dim3(64), 0, ctx->stream, a, n_lo, 0, last)
            if (r == 3) { if (NRW == 16) UAVQP_DUAL_LAUNCH(3, 8, 16); else if (NRW == 24) UAVQP_DUAL_LAUNCH(3, 16, 24); else UAVQP_DUAL_LAUNCH(3, 16, 32); }
            else { if (NRW == 16) UAVQP_DUAL_LAUNCH(4, 8, 16); else if (NRW == 24) UAVQP_DUAL_LAUNCH(4, 16, 24); else UAVQP_DUAL_LAUNCH(4, 16, 32); }
#undef UAVQP_DUAL_LAUNCH
        };
        const int nvar = Mmax - 1;
        const bool mixed = uniform_segments == 0;
        if (mixed && nvar > 16 && nvar <= 24) {
            // both shapes in one launch (corridor_dual_mixed_kernel): blocks [0, split) the 8-lane groups, the rest whole rows
            const int lds_b = 8 * uavqp::corridor_dual_mixed_lds(r);
            int wpc_d = (160 * 1024) / lds_b;
            if (wpc_d > 8) wpc_d = 8;
            const long long cap = (long long)ctx->num_cus * wpc_d;
            long long g8 = ((long long)n_traj + 7) / 8, g16 = ((long long)n_traj + 3) / 4;
            if (g8 > cap / 2) g8 = cap / 2;
            if (g16 > cap - g8) g16 = cap - g8;
            if (r == 3) hipLaunchKernelGGL((uavqp::corridor_dual_mixed_kernel<3>), dim3((unsigned)(g8 + g16)), dim3(64), 0, ctx->stream, a, (int)g8, 0);
            else hipLaunchKernelGGL((uavqp::corridor_dual_mixed_kernel<4>), dim3((unsigned)(g8 + g16)), dim3(64), 0, ctx->stream, a, (int)g8, 0);
        } else {
            // (`last`: the launch that also takes -- as invalid -- whatever is longer than any tableau)
            if (nvar <= 16 || mixed) launch_dual(8, 16, 1, nvar <= 16 ? 1 : 0);
            if (nvar > 16) launch_dual(16, nvar <= 24 ? 24 : 32, mixed ? 17 : 1, 1);
        }
    }
    if (r == 3) {
        if (ws_knots > 0) hipLaunchKernelGGL((uavqp::corridor_solve_kernel<3, true>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, a);
        else hipLaunchKernelGGL((uavqp::corridor_solve_kernel<3, false>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, a);
    } else {
        if (tail_shape) {
            if (ws_knots > 0) hipLaunchKernelGGL((uavqp::corridor_solve_kernel<4, true, 2>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, a);
            else hipLaunchKernelGGL((uavqp::corridor_solve_kernel<4, false, 2>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, a);
        } else if (ws_knots > 0) hipLaunchKernelGGL((uavqp::corridor_solve_kernel<4, true>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, a);
        else hipLaunchKernelGGL((uavqp::corridor_solve_kernel<4, false>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, a);
    }
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_solve_corridor_warm_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                                const int32_t* d_seg_offsets, const double* d_waypoints, const double* d_times,
                                                const double* d_bc, const double* d_corr_lo, const double* d_corr_hi,
                                                double* d_coeff_out, int32_t* d_status_out, int32_t* d_iters_out,
                                                uint64_t* d_active_set, int warm_start) {
    return corridor_warm_impl(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, d_times, d_bc, d_corr_lo, d_corr_hi,
                              d_coeff_out, d_status_out, d_iters_out, d_active_set, warm_start, -1);
}

#ifdef UAVQP_DUAL_DEBUG
// debug build only (tools/corridor_dual_gpu_probe.py): what corridor_dual_kernel computed for the first 64 trajectories of the last
// cold corridor solve, and the starting sets [n_traj][3][2] it handed to the solve kernel
extern "C" int uavqp_debug_corridor_dual(uavqp_ctx* ctx, double* out_64x2048, unsigned long long* out_guess, int n_traj) {
    if (!ctx || !ctx->dbg_dual) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipStreamSynchronize(ctx->stream));
    UAVQP_HIP(hipMemcpy(out_64x2048, ctx->dbg_dual, 64 * 2048 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_guess && ctx->dbg_guess) UAVQP_HIP(hipMemcpy(out_guess, ctx->dbg_guess, sizeof(unsigned long long) * 6 * (size_t)n_traj, hipMemcpyDeviceToHost));
    return UAVQP_OK;
}
#endif

#ifdef UAVQP_CORRIDOR_TIMING
// debug build only (tools/corridor_sections.py): cycles wave 0 of the last corridor solve spent per section
extern "C" int uavqp_debug_corridor_stamps(uavqp_ctx* ctx, long long* out7) {
    if (!ctx || !out7 || !ctx->ws.p) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipStreamSynchronize(ctx->stream));
    UAVQP_HIP(hipMemcpy(out7, (char*)ctx->dbg_queue + 64, 7 * sizeof(long long), hipMemcpyDeviceToHost));
    return UAVQP_OK;
}
#endif

#ifdef UAVQP_CLOUD_STATS
// probe build only (tools/cloud_phase_probe.py): blocks of the last cloud_grid2d_kernel launch that scanned ring 0 / 1 / 2
extern "C" int uavqp_debug_cloud_phases(uavqp_ctx* ctx, unsigned int* out4) {
    if (!ctx || !out4 || !ctx->dbg_queue) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipStreamSynchronize(ctx->stream));
    UAVQP_HIP(hipMemcpy(out4, ctx->dbg_queue, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost));
    return UAVQP_OK;
}
#endif

#ifdef UAVQP_LANE_TIMING
// probe build only (tools/lane_sections.py): cycles block 0 of the last corridor_dual_lane_kernel launch spent per section
extern "C" int uavqp_debug_lane_stamps(uavqp_ctx* ctx, long long* out8) {
    if (!ctx || !out8 || !ctx->dbg_queue) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipStreamSynchronize(ctx->stream));
    UAVQP_HIP(hipMemcpy(out8, (char*)ctx->dbg_queue + 128, 8 * sizeof(long long), hipMemcpyDeviceToHost));
    return UAVQP_OK;
}
#endif

#ifdef UAVQP_ROWS2_TIMING
// probe build only (tools/rows_sections.py): cycles wave 0 of the last pair-kernel rows solve spent per section
extern "C" int uavqp_debug_rows2_stamps(uavqp_ctx* ctx, long long* out8) {
    if (!ctx || !out8 || !ctx->dbg_queue) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipStreamSynchronize(ctx->stream));
    UAVQP_HIP(hipMemcpy(out8, (char*)ctx->dbg_queue + 64, 8 * sizeof(long long), hipMemcpyDeviceToHost));
    return UAVQP_OK;
}
#endif

#ifdef G2_TIMING
// (probe build) s_memtime stamps of wave 0 of the last ragged pair-kernel launch: tools/generic2_sections.py
extern "C" int uavqp_debug_generic2_stamps(uavqp_ctx* ctx, long long* out9) {
    if (!ctx || !out9) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipStreamSynchronize(ctx->stream));
    UAVQP_HIP(hipMemcpy(out9, (char*)ctx->dummy + 1024, 15 * sizeof(long long), hipMemcpyDeviceToHost));
    return UAVQP_OK;
}
#endif

#ifdef UAVQP_DUAL_DEBUG
static double* g_rows_dbg = nullptr;   // dump area of rows_dual_kernel (tools/rows_dual_gpu_probe.py)
#endif
static int rows_batch_impl(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                           const int32_t* d_seg_offsets, const double* d_waypoints, const double* d_times,
                           const double* d_bc, const double* d_corr_lo, const double* d_corr_hi, int rows_per_segment,
                           const double* d_row_tau, const int32_t* d_row_deriv, const double* d_row_lo,
                           const double* d_row_hi, double* d_coeff_out, int32_t* d_status_out, int32_t* d_iters_out,
                           uint64_t* d_active_out, long long total_segments) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || (rows_per_segment != 1 && rows_per_segment != 2))
        return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!d_waypoints || !d_times || !d_bc || !d_coeff_out || !d_status_out || !d_row_tau || !d_row_deriv || !d_row_lo || !d_row_hi)
        return UAVQP_ERR_INVALID_ARG;
    if ((d_corr_lo == nullptr) != (d_corr_hi == nullptr)) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && (!d_seg_offsets || max_segments < 1)) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const int Mmax = uniform_segments > 0 ? uniform_segments : max_segments;
    long long rows = 0;   // (an unknown total is read back once here, handed on to the box phase below)
    int rc = batch_rows(ctx, n_traj, uniform_segments, total_segments, d_seg_offsets, &rows);
    if (rc != UAVQP_OK) return rc;
    // Phase 1 (only with knot boxes): the box-only problem on the fast corridor kernel; its working set is where the dual method
    // starts, so that its iterations go into the rows and the few boxes they move instead of re-discovering every active box one
    // constraint per block solve (BASELINE config 3 with K = 2 rows: 34 -> 25 iterations mean, 36 -> 30 ms; uavqp_settings.warm_start = 0
    // starts from the empty set).
    const bool warm = d_corr_lo != nullptr && ctx->settings.warm_start != 0;
    const int K_ = rows_per_segment;
    const int K = rows_per_segment, Bk = r + K;
    const bool pair_kernel = ctx->settings.rows_lanes_per_problem != 1;
    // Round 4: the starting set of boxes AND rows from the position-space dual method on the refined time grid (qp_rows_dual.h: a row is a
    // bound on a component of a knot inserted at its time); trajectories it does not take (rows at tau = 0, too many constraints) go
    // through the box phase as before.  uavqp_settings.corridor_initial_guess != 2 or warm_start = 0 switch it off.
    const bool prelude = ctx->settings.corridor_initial_guess == 2 && ctx->settings.warm_start != 0 && pair_kernel &&
                         Mmax >= 2 && (Mmax - 1) + K_ * Mmax <= 48;
    if (warm || prelude) {
        rc = dev_grow(ctx->stream, ctx->rows_warm, sizeof(uint64_t) * (size_t)n_traj * 6);
        if (rc != UAVQP_OK) return rc;
    }
    unsigned long long* const d_warm_box = (warm || prelude) ? (unsigned long long*)ctx->rows_warm.p : nullptr;
    const long long total_seg = rows - n_traj;
    const long long pairs = 3LL * n_traj;
    unsigned long long* d_warm_rows = nullptr;
    unsigned char* d_need_phase1 = nullptr;
    double* d_gfun_pre = nullptr;
    unsigned int* d_n_phase1 = nullptr;
    unsigned int* d_queue = nullptr;
    unsigned long long* d_desc = nullptr;
    int32_t* d_status_box = nullptr;
    double *d_kdF = nullptr, *d_kdB = nullptr;
    long long kd_plane = 0;
    uavqp::RowsArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.max_segments = Mmax;
    a.max_iter = ctx->settings.max_iter > 0 ? ctx->settings.max_iter : 12 * Mmax * (1 + K) + 30;
    a.eps_prim_inf = ctx->settings.eps_prim_inf;
    a.seg_offsets = d_seg_offsets; a.waypoints = d_waypoints; a.times = d_times; a.bc = d_bc;
    a.corr_lo = d_corr_lo; a.corr_hi = d_corr_hi; a.row_tau = d_row_tau; a.row_deriv = d_row_deriv; a.row_lo = d_row_lo; a.row_hi = d_row_hi;
    a.status = d_status_out; a.iters = d_iters_out; a.active = (unsigned long long*)d_active_out;
    a.xsol = nullptr; a.ws = nullptr; a.queue = nullptr; a.warm = nullptr; a.warm_rows = nullptr;
    uavqp::Rows2Args aa{};
    if (pair_kernel) {
        // Round 6: everything the step keeps across its launches lives in ONE persistent allocation (rows_warm2: the box phase in the middle
        // re-uses ctx->ws), and rows_prep_kernel is the step's FIRST kernel: validation + permanent masks as before, and with them the row
        // functionals (was rows_gfun_kernel: a second pass over the same rows), the initial status / iteration counts (was fill_i32_kernel + a
        // memset) and the clearing of what the prelude only writes for the trajectories it takes (was two memsets).
        Carve c;
        const int i_wr = c.add(sizeof(uint64_t) * (size_t)n_traj * 3 * 2 * K_, prelude), i_np = c.add((size_t)n_traj, prelude);
        const int i_ctr = c.add(512);   // [0, 256): the prelude's counters (its ticket: word 16); [256, 512): the pair kernel's queue
        const int i_gf = c.add(sizeof(double) * (size_t)total_seg * K_ * 2 * r);                   // row functionals: made once, used by the prelude AND the rows kernel
        // chain records (rows_chain_kernel): two halves, knot-major planes of n_traj (padded to whole waves) rows each, knots 1 .. Mmax - 1 <= 31
        const int kd_planes = Mmax - 1 < 1 ? 1 : (Mmax - 1 > 31 ? 31 : Mmax - 1);
        kd_plane = ((long long)n_traj + 63) / 64 * 64 * uavqp::rows_chain_half_mem(r);
        const size_t b_kd_half = sizeof(double) * (size_t)kd_planes * (size_t)kd_plane;
        const int i_kdF = c.add(b_kd_half, prelude), i_kdB = c.add(b_kd_half, prelude);
        const int i_desc = c.add(sizeof(unsigned long long) * (size_t)pairs * (2 + 2 * K));
        const int i_sb = c.add(sizeof(int32_t) * (size_t)n_traj, warm);                            // the box phase's statuses (not the step's)
        rc = carve_on(ctx->stream, ctx->rows_warm2, c);
        if (rc != UAVQP_OK) return rc;
        d_warm_rows = c.at<unsigned long long>(i_wr);
        d_need_phase1 = c.at<unsigned char>(i_np);
        d_n_phase1 = c.at<unsigned int>(i_ctr); d_queue = (unsigned int*)((char*)d_n_phase1 + 256);
        d_gfun_pre = c.at<double>(i_gf);
        d_kdF = c.at<double>(i_kdF); d_kdB = c.at<double>(i_kdB);
        d_desc = c.at<unsigned long long>(i_desc);
        d_status_box = c.at<int32_t>(i_sb);
        a.queue = d_queue;
        ctx->dbg_queue = a.queue;
        aa.r = a;
        aa.desc = d_desc; aa.gfun = d_gfun_pre; aa.prep_gfun = 1;
        aa.init_warm_box = d_warm_box;
        aa.init_warm_rows = d_warm_rows;
        aa.init_counters = d_n_phase1;                      // 128 words: the prelude's counters and the queue behind them
        // rows_prep_kernel: four waves per block; two trajectories per wave when none has more than 31 segments (a half-wave's lanes), else one
        const int tw = Mmax <= 31 ? 2 : 1;
        long long pgrid = ((long long)n_traj + 4 * tw - 1) / (4 * tw);
        if (pgrid > (long long)ctx->num_cus * 16) pgrid = (long long)ctx->num_cus * 16;
#define UAVQP_PREP_LAUNCH(R_, K_) do { if (tw == 2) hipLaunchKernelGGL((uavqp::rows_prep_kernel<R_, K_, 2>), dim3((unsigned)pgrid), dim3(256), 0, ctx->stream, aa); \
                                       else hipLaunchKernelGGL((uavqp::rows_prep_kernel<R_, K_, 1>), dim3((unsigned)pgrid), dim3(256), 0, ctx->stream, aa); } while (0)
        if (r == 3 && K == 1) UAVQP_PREP_LAUNCH(3, 1);
        else if (r == 3) UAVQP_PREP_LAUNCH(3, 2);
        else if (K == 1) UAVQP_PREP_LAUNCH(4, 1);
        else UAVQP_PREP_LAUNCH(4, 2);
#undef UAVQP_PREP_LAUNCH
    }
    if (prelude) {
        uavqp::RowsDualArgs da{};
        da.r.n_traj = n_traj; da.r.uniform = uniform_segments; da.r.max_segments = Mmax;
        da.r.seg_offsets = d_seg_offsets; da.r.waypoints = d_waypoints; da.r.times = d_times; da.r.bc = d_bc;
        da.r.corr_lo = d_corr_lo; da.r.corr_hi = d_corr_hi; da.r.row_tau = d_row_tau; da.r.row_deriv = d_row_deriv; da.r.row_lo = d_row_lo; da.r.row_hi = d_row_hi;
        da.order = nullptr;
        da.warm_box = d_warm_box; da.warm_rows = d_warm_rows; da.need_phase1 = d_need_phase1; da.gfun = d_gfun_pre;
        da.kdF = d_kdF; da.kdB = d_kdB; da.kd_plane = kd_plane; da.n_phase1 = d_n_phase1;
        da.ticket = (d_n_phase1 && ctx->deal_tickets) ? d_n_phase1 + 16 : nullptr;      // (the prelude's counter block: zeroed by rows_prep_kernel, the step's first kernel)
        {   // the chain of every trajectory once, one lane each (the prelude's waves would each repeat it in 64 lanes)
            long long cg = ((long long)n_traj + 63) / 64;
            if (cg > (long long)ctx->num_cus * 16) cg = (long long)ctx->num_cus * 16;
            if (r == 3) hipLaunchKernelGGL((uavqp::rows_chain_kernel<3>), dim3((unsigned)cg), dim3(64), 0, ctx->stream, da.r, d_kdF, d_kdB, kd_plane);
            else hipLaunchKernelGGL((uavqp::rows_chain_kernel<4>), dim3((unsigned)cg), dim3(64), 0, ctx->stream, da.r, d_kdF, d_kdB, kd_plane);
        }
#ifdef UAVQP_DUAL_DEBUG
        {
            if (!g_rows_dbg) { UAVQP_HIP(hipMalloc(&g_rows_dbg, 64 * 2048 * sizeof(double))); }   // (the size uavqp_debug_corridor_dual copies)
            UAVQP_HIP(hipMemsetAsync(g_rows_dbg, 0, 64 * 2048 * sizeof(double), ctx->stream));
            da.dbg = g_rows_dbg;
        }
#endif
        // one trajectory per wave; waves per CU by the LDS of a block (two per SIMD at most: 256 registers)
        int wpc_r = (160 * 1024) / (8 * uavqp::rows_dual_lds_doubles(r));
        if (wpc_r > 8) wpc_r = 8;
        const long long dgrid = (long long)n_traj < (long long)ctx->num_cus * wpc_r ? (long long)n_traj : (long long)ctx->num_cus * wpc_r;
        if (r == 3 && K_ == 1) hipLaunchKernelGGL((uavqp::rows_dual_kernel<3, 1>), dim3((unsigned)dgrid), dim3(64), 0, ctx->stream, da, 0);
        else if (r == 3) hipLaunchKernelGGL((uavqp::rows_dual_kernel<3, 2>), dim3((unsigned)dgrid), dim3(64), 0, ctx->stream, da, 0);
        else if (K_ == 1) hipLaunchKernelGGL((uavqp::rows_dual_kernel<4, 1>), dim3((unsigned)dgrid), dim3(64), 0, ctx->stream, da, 0);
        else hipLaunchKernelGGL((uavqp::rows_dual_kernel<4, 2>), dim3((unsigned)dgrid), dim3(64), 0, ctx->stream, da, 0);
    }
    if (warm && !prelude) {
        // The box phase -- only WITHOUT the prelude.  (Round 6: with it, what the prelude does not take is, by the host's own admission test
        // (Mmax - 1) + K Mmax <= 48, exactly what rows_prep_kernel flags as invalid input -- bad durations, bad rows -- or a single segment, which has no
        // knot box to start from: the three launches that compacted and solved that list -- empty as a rule -- are gone; need_phase1 is still written,
        // nobody reads it.)  The box phase's statuses are its own: the step's statuses started in rows_prep_kernel.
        const int rc1 = corridor_warm_impl(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, d_times,
                                           d_bc, d_corr_lo, d_corr_hi, d_coeff_out, pair_kernel ? d_status_box : d_status_out, nullptr, (uint64_t*)d_warm_box, 0, rows - n_traj);
        if (rc1 != UAVQP_OK) return rc1;
    }
#ifdef UAVQP_DUAL_DEBUG
    if (prelude) {   // (after the box phase, which points these at its own dump)
        static unsigned long long* s_box = nullptr;
        static size_t s_box_n = 0;
        if (s_box_n < (size_t)n_traj * 6) { if (s_box) (void)hipFree(s_box); UAVQP_HIP(hipMalloc((void**)&s_box, sizeof(uint64_t) * (size_t)n_traj * 6)); s_box_n = (size_t)n_traj * 6; }
        UAVQP_HIP(hipMemcpyAsync(s_box, d_warm_box, sizeof(uint64_t) * (size_t)n_traj * 6, hipMemcpyDeviceToDevice, ctx->stream));
        ctx->dbg_guess = s_box;
        ctx->dbg_dual = g_rows_dbg;
    }
#endif
    a.warm = d_warm_box;
    a.warm_rows = prelude ? (const unsigned long long*)d_warm_rows : nullptr;
    if (pair_kernel) {
        // two lanes per problem, sweep state in LDS (qp_rows2.h): 80 KiB per single-wave workgroup = two waves per CU
        const int Fp = Bk * (Bk + 1) / 2 + Bk, NCN = 1 + K;
        const int kown = (Mmax + 1) / 2;                       // own knots of the longer half, meeting knot included = state slots 0..kown-1
        // the general passes keep 80 KiB of sweep records per wave (two waves per CU); the verifying pass 40 KiB (four: one per SIMD) and the rest in
        // the HBM workspace -- each pass has its own count of workspace knots and its own grid
        // (the verifying pass also keeps rows2_reg_knots() slots in registers -- unless the batch needs workspace slots anyway: that instantiation has none)
        const int NT = uavqp::rows2_lds_knots(r, K, false), NTv = uavqp::rows2_lds_knots(r, K, true);
        const int ws_knots = kown > NT ? kown - NT : 0, ws_knots_v = kown > NTv + uavqp::rows2_reg_knots(true) ? kown - NTv : 0;
        long long grid = (pairs + 31) / 32, grid_v = grid;
        const long long max_grid = (long long)ctx->num_cus * uavqp::rows2_waves_per_cu(false), max_grid_v = (long long)ctx->num_cus * uavqp::rows2_waves_per_cu(true);
        if (grid > max_grid) grid = max_grid;
        if (grid_v > max_grid_v) grid_v = max_grid_v;
        const bool deal_by_length = uniform_segments == 0 && n_traj >= 64 && ctx->settings.ragged_window_sort;
        const size_t b_state_g = sizeof(double) * (size_t)ws_knots * Fp * (size_t)grid * 64, b_state_v = prelude ? sizeof(double) * (size_t)ws_knots_v * Fp * (size_t)grid_v * 64 : 0;
        Carve c;
        (void)c.add(256);   // unused head: no kernel is handed these bytes (the pair kernel's queue is in rows_warm2); kept: the same bytes are asked for
        const LengthOrder i_order = length_order_slots(c, n_traj, deal_by_length);
        const int i_state = c.add(b_state_g > b_state_v ? b_state_g : b_state_v);
        const int i_lam = c.add(sizeof(double) * (size_t)kown * 2 * NCN * (size_t)grid * 64);
        const int i_redo = c.add(sizeof(unsigned int) * (size_t)pairs);
        rc = carve_on(ctx->stream, ctx->ws, c);
        if (rc != UAVQP_OK) return rc;
        aa.order = nullptr;
        if (deal_by_length) {
            rc = make_length_order(ctx, d_seg_offsets, n_traj, c, i_order, &aa.order);
            if (rc != UAVQP_OK) return rc;
        }
        a.ws = c.at<double>(i_state);
        aa.lam = c.at<double>(i_lam);
        aa.redo = c.at<unsigned int>(i_redo);
        aa.ws_knots = ws_knots;
        aa.lam_knots = kown;
        aa.coeff = d_coeff_out;                                 // the pair kernels write the polynomials themselves: no xsol, no emission launch
        aa.prep_gfun = 0; aa.init_warm_box = nullptr; aa.init_warm_rows = nullptr; aa.init_counters = nullptr;
        aa.r = a;
        // first pass: every problem.  With the prelude's starting sets it is the VERIFYING pass (one block solve, no dual state in HBM; what it
        // does not confirm goes to the redo list); without them the general first pass.  Second pass (Goldfarb-Idnani's dependent-constraint
        // route, and every problem the verifying pass handed on): the redo list -- empty as a rule (one wave per CU then; behind the
        // verifying pass the full grid: its list may be long when the prelude did not take the batch)
        const long long grid2 = prelude ? grid : (grid < (long long)ctx->num_cus ? grid : (long long)ctx->num_cus);
        uavqp::Rows2Args av = aa;                               // the verifying pass: its own workspace split
        av.ws_knots = ws_knots_v;
#define UAVQP_ROWS2(RR, KK)                                                                                                                  \
    do {                                                                                                                                     \
        if (prelude) {                                                                                                                      \
            if (ws_knots_v > 0) hipLaunchKernelGGL((uavqp::rows_pair_kernel<RR, KK, true, false, true>), dim3((unsigned)grid_v), dim3(64), 0, ctx->stream, av); \
            else hipLaunchKernelGGL((uavqp::rows_pair_kernel<RR, KK, false, false, true>), dim3((unsigned)grid_v), dim3(64), 0, ctx->stream, av);               \
        } else if (ws_knots > 0) {                                                                                                          \
            hipLaunchKernelGGL((uavqp::rows_pair_kernel<RR, KK, true, false, false>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, aa);  \
        } else {                                                                                                                            \
            hipLaunchKernelGGL((uavqp::rows_pair_kernel<RR, KK, false, false, false>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, aa); \
        }                                                                                                                                   \
        if (ws_knots > 0) hipLaunchKernelGGL((uavqp::rows_pair_kernel<RR, KK, true, true, false>), dim3((unsigned)grid2), dim3(64), 0, ctx->stream, aa); \
        else hipLaunchKernelGGL((uavqp::rows_pair_kernel<RR, KK, false, true, false>), dim3((unsigned)grid2), dim3(64), 0, ctx->stream, aa);           \
    } while (0)
        if (r == 3 && K == 1) UAVQP_ROWS2(3, 1);
        else if (r == 3) UAVQP_ROWS2(3, 2);
        else if (K == 1) UAVQP_ROWS2(4, 1);
        else UAVQP_ROWS2(4, 2);
#undef UAVQP_ROWS2
    } else {
        const int F = Bk * (Bk + 1) / 2 + Bk + 2 * (1 + K);   // must match rows_solve_kernel's state layout
        long long grid = (3LL * n_traj + 63) / 64;
        const long long max_grid = (long long)ctx->num_cus * 4;
        if (grid > max_grid) grid = max_grid;
        Carve c;
        const int i_xsol = c.add(sizeof(double) * 3 * (size_t)r * (size_t)rows), i_queue = c.add(256);
        const int i_state = c.add(sizeof(double) * (size_t)Mmax * F * (size_t)grid * 64);
        rc = carve_on(ctx->stream, ctx->ws, c);
        if (rc != UAVQP_OK) return rc;
        a.xsol = c.at<double>(i_xsol); a.queue = c.at<unsigned int>(i_queue); a.ws = c.at<double>(i_state);
        UAVQP_HIP(hipMemsetAsync(a.queue, 0, 256, ctx->stream));
        hipLaunchKernelGGL(uavqp::fill_i32_kernel, dim3((n_traj + 255) / 256), dim3(256), 0, ctx->stream, d_status_out, n_traj, (int32_t)UAVQP_SOLVED);
        if (d_iters_out) UAVQP_HIP(hipMemsetAsync(d_iters_out, 0, sizeof(int32_t) * (size_t)n_traj, ctx->stream));
        if (r == 3) {
            if (K == 1) hipLaunchKernelGGL((uavqp::rows_solve_kernel<3, 1>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, a);
            else hipLaunchKernelGGL((uavqp::rows_solve_kernel<3, 2>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, a);
        } else {
            if (K == 1) hipLaunchKernelGGL((uavqp::rows_solve_kernel<4, 1>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, a);
            else hipLaunchKernelGGL((uavqp::rows_solve_kernel<4, 2>), dim3((unsigned)grid), dim3(64), 0, ctx->stream, a);
        }
        // Hermite solution -> coefficients (the corridor solver's emission kernel; it reads the same fields) -- the one-lane cross-check kernel only
        uavqp::CorridorArgs e{};
        e.n_traj = n_traj; e.uniform = uniform_segments; e.max_segments = Mmax; e.seg_offsets = d_seg_offsets; e.waypoints = d_waypoints;
        e.times = d_times; e.bc = d_bc; e.coeff = d_coeff_out; e.status = d_status_out; e.xsol = a.xsol;
        const long long chunks = 3LL * (rows - n_traj);
        long long egrid = (chunks + 255) / 256;
        if (egrid > (long long)ctx->num_cus * 16) egrid = (long long)ctx->num_cus * 16;
        if (chunks > 0) {
            if (r == 3) hipLaunchKernelGGL((uavqp::corridor_emit_kernel<3>), dim3((unsigned)egrid), dim3(256), 0, ctx->stream, e, chunks);
            else hipLaunchKernelGGL((uavqp::corridor_emit_kernel<4>), dim3((unsigned)egrid), dim3(256), 0, ctx->stream, e, chunks);
        }
    }
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_solve_rows_batch_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                             const int32_t* d_seg_offsets, const double* d_waypoints, const double* d_times,
                                             const double* d_bc, const double* d_corr_lo, const double* d_corr_hi, int rows_per_segment,
                                             const double* d_row_tau, const int32_t* d_row_deriv, const double* d_row_lo,
                                             const double* d_row_hi, double* d_coeff_out, int32_t* d_status_out, int32_t* d_iters_out,
                                             uint64_t* d_active_out) {
    return rows_batch_impl(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, d_times, d_bc, d_corr_lo, d_corr_hi,
                           rows_per_segment, d_row_tau, d_row_deriv, d_row_lo, d_row_hi, d_coeff_out, d_status_out, d_iters_out, d_active_out, -1);
}

extern "C" int uavqp_solve_corridor_batch_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                                 const int32_t* d_seg_offsets, const double* d_waypoints, const double* d_times,
                                                 const double* d_bc, const double* d_corr_lo, const double* d_corr_hi,
                                                 double* d_coeff_out, int32_t* d_status_out, int32_t* d_iters_out) {
    return uavqp_solve_corridor_warm_device(ctx, r, n_traj, uniform_segments, max_segments, d_seg_offsets, d_waypoints, d_times, d_bc,
                                            d_corr_lo, d_corr_hi, d_coeff_out, d_status_out, d_iters_out, nullptr, 0);
}

extern "C" int uavqp_solve_corridor_batch_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                               const int32_t* seg_offsets, const double* waypoints, const double* times,
                                               const double* bc, const double* corr_lo, const double* corr_hi,
                                               double* coeff_out, int32_t* status_out, int32_t* iters_out) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0) return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!waypoints || !times || !bc || !corr_lo || !corr_hi || !coeff_out) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && !seg_offsets) return UAVQP_ERR_INVALID_ARG;
    BatchShape sh;
    int rc = batch_shape(n_traj, uniform_segments, max_segments, seg_offsets, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg, b_wp = sizeof(double) * 3 * (tot + n);
    Stage st;
    const int i_off = uniform_segments > 0 ? -1 : st.in(seg_offsets, sizeof(int32_t) * (n + 1));
    const int i_wp = st.in(waypoints, b_wp), i_lo = st.in(corr_lo, b_wp), i_hi = st.in(corr_hi, b_wp);
    const int i_t = st.in(times, sizeof(double) * tot);
    const int i_bc = st.in(bc, sizeof(double) * n * 2 * (r - 1) * 3);
    const int i_out = st.out(coeff_out, sizeof(double) * 3 * 2 * r * tot, true);
    const int i_st = st.out(status_out, sizeof(int32_t) * n), i_it = st.out(iters_out, sizeof(int32_t) * n);
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = corridor_warm_impl(ctx, r, n_traj, uniform_segments, sh.Mmax, st.at<int32_t>(i_off), st.at<double>(i_wp), st.at<double>(i_t),
                            st.at<double>(i_bc), st.at<double>(i_lo), st.at<double>(i_hi), st.at<double>(i_out), st.at<int32_t>(i_st),
                            st.at<int32_t>(i_it), nullptr, 0, sh.total_seg);
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_solve_corridor_batch_host");
}

extern "C" int uavqp_solve_rows_batch_host(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, int max_segments,
                                           const int32_t* seg_offsets, const double* waypoints, const double* times, const double* bc,
                                           const double* corr_lo, const double* corr_hi, int rows_per_segment, const double* row_tau,
                                           const int32_t* row_deriv, const double* row_lo, const double* row_hi, double* coeff_out,
                                           int32_t* status_out, int32_t* iters_out) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || (rows_per_segment != 1 && rows_per_segment != 2))
        return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!waypoints || !times || !bc || !coeff_out || !row_tau || !row_deriv || !row_lo || !row_hi) return UAVQP_ERR_INVALID_ARG;
    if ((corr_lo == nullptr) != (corr_hi == nullptr)) return UAVQP_ERR_INVALID_ARG;
    if (uniform_segments == 0 && !seg_offsets) return UAVQP_ERR_INVALID_ARG;
    BatchShape sh;
    int rc = batch_shape(n_traj, uniform_segments, max_segments, seg_offsets, &sh);
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    const int K = rows_per_segment;
    const size_t n = (size_t)n_traj, tot = (size_t)sh.total_seg, b_wp = sizeof(double) * 3 * (tot + n), n_row = tot * K;
    Stage st;
    const int i_off = uniform_segments > 0 ? -1 : st.in(seg_offsets, sizeof(int32_t) * (n + 1));
    const int i_wp = st.in(waypoints, b_wp);
    const int i_lo = corr_lo ? st.in(corr_lo, b_wp) : -1, i_hi = corr_lo ? st.in(corr_hi, b_wp) : -1;   // (no knot boxes: waypoint equalities)
    const int i_t = st.in(times, sizeof(double) * tot);
    const int i_bc = st.in(bc, sizeof(double) * n * 2 * (r - 1) * 3);
    const int i_rt = st.in(row_tau, sizeof(double) * n_row), i_rd = st.in(row_deriv, sizeof(int32_t) * n_row);
    const int i_rl = st.in(row_lo, sizeof(double) * 3 * n_row), i_rh = st.in(row_hi, sizeof(double) * 3 * n_row);
    const int i_out = st.out(coeff_out, sizeof(double) * 3 * 2 * r * tot, true);
    const int i_st = st.out(status_out, sizeof(int32_t) * n), i_it = st.out(iters_out, sizeof(int32_t) * n);
    rc = stage_begin(ctx, st);
    if (rc != UAVQP_OK) return rc;
    rc = rows_batch_impl(ctx, r, n_traj, uniform_segments, sh.Mmax, st.at<int32_t>(i_off), st.at<double>(i_wp), st.at<double>(i_t),
                         st.at<double>(i_bc), st.at<double>(i_lo), st.at<double>(i_hi), K, st.at<double>(i_rt), st.at<int32_t>(i_rd),
                         st.at<double>(i_rl), st.at<double>(i_rh), st.at<double>(i_out), st.at<int32_t>(i_st), st.at<int32_t>(i_it), nullptr,
                         sh.total_seg);
    if (rc != UAVQP_OK) return rc;
    return stage_end(ctx, st, "uavqp_solve_rows_batch_host");
}

static int time_reallocate_impl(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                double* d_times, const double* d_coeff, double v_max, double a_max,
                                int samples_per_seg, double max_stretch, int32_t* d_changed_out, double* d_scale_acc,
                                const int32_t* d_list = nullptr, const int* d_n_list = nullptr);
extern "C" int uavqp_time_reallocate_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                            double* d_times, const double* d_coeff, double v_max, double a_max,
                                            int samples_per_seg, double max_stretch, int32_t* d_changed_out) {
    return time_reallocate_impl(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, v_max, a_max, samples_per_seg, max_stretch, d_changed_out, nullptr);
}
static int time_reallocate_impl(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                double* d_times, const double* d_coeff, double v_max, double a_max,
                                int samples_per_seg, double max_stretch, int32_t* d_changed_out, double* d_scale_acc,
                                const int32_t* d_list, const int* d_n_list) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || uniform_segments < 0 || !(v_max > 0.0) || !(a_max > 0.0) ||
        samples_per_seg < 1 || !(max_stretch > 1.0))
        return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!d_times || !d_coeff || (uniform_segments == 0 && !d_seg_offsets)) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    uavqp::ReallocArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.samples = samples_per_seg;
    a.seg_offsets = d_seg_offsets; a.times = d_times; a.coeff = d_coeff; a.v_max = v_max; a.a_max = a_max;
    a.max_stretch = max_stretch; a.changed = d_changed_out; a.scale_acc = d_scale_acc;
    a.list = d_list; a.n_list = d_list ? d_n_list : nullptr;
    a.dead_band = ctx->settings.realloc_dead_band; a.overshoot = ctx->settings.realloc_overshoot;
    long long grid_ll = ((long long)n_traj * 8 + 63) / 64;  // 8 lanes per trajectory
    if (grid_ll > (long long)ctx->num_cus * 32) grid_ll = (long long)ctx->num_cus * 32;
    const int grid = (int)grid_ll;
    if (r == 3)
        hipLaunchKernelGGL(uavqp::realloc_kernel<3>, dim3(grid), dim3(64), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::realloc_kernel<4>, dim3(grid), dim3(64), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_ellipsoid_check_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                            const double* d_times, const double* d_coeff, int n_samples, double t0, double dt,
                                            const double* d_obstacles, int n_obs, double robot_r, double robot_h,
                                            int32_t* d_first_hit, uint8_t* d_flags) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || n_samples < 0 || uniform_segments < 0 || n_obs < 0 || !(robot_r > 0.0) || !(robot_h > 0.0))
        return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!d_times || !d_coeff || !d_first_hit || (n_obs > 0 && !d_obstacles) || (uniform_segments == 0 && !d_seg_offsets))
        return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(uavqp::fill_i32_kernel, dim3((n_traj + 255) / 256), dim3(256), 0, ctx->stream, d_first_hit, n_traj, (int32_t)n_samples);
    if (n_samples == 0) return UAVQP_OK;
    uavqp::EllipsoidArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.n_samples = n_samples; a.n_obs = n_obs;
    a.seg_offsets = d_seg_offsets; a.times = d_times; a.coeff = d_coeff; a.obs = d_obstacles;
    a.t0 = t0; a.dt = dt; a.robot_r = robot_r; a.robot_h = robot_h; a.first_hit = d_first_hit; a.flags = d_flags;
    const long long total = (long long)n_traj * n_samples;
    long long grid = (total + 255) / 256;
    if (grid > (long long)ctx->num_cus * 16) grid = (long long)ctx->num_cus * 16;
    if (r == 3)
        hipLaunchKernelGGL(uavqp::ellipsoid_kernel<3>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::ellipsoid_kernel<4>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

// ---- obstacle grid (uniform cells over the cloud) + grid-accelerated ellipsoid check ------------------------------
struct uavqp_grid {
    int device = 0;
    int n_obs = 0;
    uavqp::GridView view{};
    int32_t* d_cell_start = nullptr;
    double* d_pts = nullptr;
};

extern "C" int uavqp_obstacle_grid_destroy(uavqp_ctx* ctx, uavqp_grid* grid) {
    if (!grid) return UAVQP_OK;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    (void)hipSetDevice(grid->device);
    if (grid->d_cell_start) (void)hipFree(grid->d_cell_start);
    if (grid->d_pts) (void)hipFree(grid->d_pts);
    delete grid;
    return UAVQP_OK;
}

extern "C" int uavqp_obstacle_grid_build_device(uavqp_ctx* ctx, const double* d_obstacles, int n_obs, double cell_size,
                                                uavqp_grid** out_grid) {
    if (!ctx || !out_grid || n_obs < 0 || (n_obs > 0 && !d_obstacles) || !(cell_size > 0.0) || !(cell_size < INFINITY))
        return UAVQP_ERR_INVALID_ARG;
    *out_grid = nullptr;
    UAVQP_HIP(hipSetDevice(ctx->device));
    uavqp_grid* g = new (std::nothrow) uavqp_grid();
    if (!g) return UAVQP_ERR_ALLOC;
    g->device = ctx->device;
    g->n_obs = n_obs;
    hipStream_t s = ctx->stream;
    double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    int rc = UAVQP_OK;
    double* d_part = nullptr;
    int32_t* d_cell_of = nullptr;
    int32_t* d_cursor = nullptr;
    std::vector<int32_t> h_counts;
#define UAVQP_GRID_HIP(expr)                                                                     \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            g_last_error = std::string(#expr) + ": " + hipGetErrorString(e_);                    \
            rc = UAVQP_ERR_HIP;                                                                  \
            goto fail;                                                                           \
        }                                                                                        \
    } while (0)
    {
        if (n_obs > 0) {
            const int nb = std::min(256, (n_obs + 255) / 256);
            UAVQP_GRID_HIP(hipMalloc((void**)&d_part, sizeof(double) * 6 * nb));
            hipLaunchKernelGGL(uavqp::grid_bounds_kernel, dim3(nb), dim3(256), 0, s, d_obstacles, n_obs, d_part);
            std::vector<double> part(6 * (size_t)nb);
            UAVQP_GRID_HIP(hipMemcpyAsync(part.data(), d_part, sizeof(double) * 6 * nb, hipMemcpyDeviceToHost, s));
            UAVQP_GRID_HIP(hipStreamSynchronize(s));
            for (int ax = 0; ax < 3; ++ax) { mn[ax] = INFINITY; mx[ax] = -INFINITY; }
            for (int b = 0; b < nb; ++b)
                for (int ax = 0; ax < 3; ++ax) {
                    mn[ax] = std::fmin(mn[ax], part[6 * b + ax]);
                    mx[ax] = std::fmax(mx[ax], part[6 * b + 3 + ax]);
                }
            for (int ax = 0; ax < 3; ++ax)
                if (!(mn[ax] > -INFINITY) || !(mx[ax] < INFINITY) || mn[ax] != mn[ax]) {
                    g_last_error = "obstacle cloud contains non-finite coordinates";
                    rc = UAVQP_ERR_INVALID_ARG;
                    goto fail;
                }
        }
        // cells: at most 2^22; a cloud too large for the requested cell size gets proportionally larger cells
        double cell = cell_size;
        long long dims[3];
        for (;;) {
            long long n = 1;
            for (int ax = 0; ax < 3; ++ax) {
                dims[ax] = (long long)std::floor((mx[ax] - mn[ax]) / cell) + 1;
                n *= dims[ax];
            }
            if (n <= (1ll << 22)) break;
            cell *= 2.0;
        }
        const int ncell = (int)(dims[0] * dims[1] * dims[2]);
        for (int ax = 0; ax < 3; ++ax) { g->view.org[ax] = mn[ax]; g->view.dim[ax] = (int)dims[ax]; }
        g->view.inv_cell = 1.0 / cell;
        UAVQP_GRID_HIP(hipMalloc((void**)&g->d_cell_start, sizeof(int32_t) * (size_t)(ncell + 1)));
        UAVQP_GRID_HIP(hipMalloc((void**)&g->d_pts, sizeof(double) * 3 * (size_t)(n_obs > 0 ? n_obs : 1)));
        UAVQP_GRID_HIP(hipMemsetAsync(g->d_cell_start, 0, sizeof(int32_t) * (size_t)(ncell + 1), s));
        if (n_obs > 0) {
            UAVQP_GRID_HIP(hipMalloc((void**)&d_cell_of, sizeof(int32_t) * (size_t)n_obs));
            UAVQP_GRID_HIP(hipMalloc((void**)&d_cursor, sizeof(int32_t) * (size_t)(ncell + 1)));
            // counts land in cell_start[c + 1] so that the host prefix leaves an exclusive scan in place
            hipLaunchKernelGGL(uavqp::grid_count_kernel, dim3((n_obs + 255) / 256), dim3(256), 0, s, g->view, d_obstacles, n_obs,
                               d_cell_of, g->d_cell_start + 1);
            h_counts.resize((size_t)ncell + 1);
            UAVQP_GRID_HIP(hipMemcpyAsync(h_counts.data(), g->d_cell_start, sizeof(int32_t) * (size_t)(ncell + 1), hipMemcpyDeviceToHost, s));
            UAVQP_GRID_HIP(hipStreamSynchronize(s));
            for (int c = 0; c < ncell; ++c) h_counts[c + 1] += h_counts[c];
            UAVQP_GRID_HIP(hipMemcpyAsync(g->d_cell_start, h_counts.data(), sizeof(int32_t) * (size_t)(ncell + 1), hipMemcpyHostToDevice, s));
            UAVQP_GRID_HIP(hipMemcpyAsync(d_cursor, h_counts.data(), sizeof(int32_t) * (size_t)(ncell + 1), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(uavqp::grid_scatter_kernel, dim3((n_obs + 255) / 256), dim3(256), 0, s, d_obstacles, n_obs, d_cell_of,
                               d_cursor, g->d_pts);
            UAVQP_GRID_HIP(hipGetLastError());
            UAVQP_GRID_HIP(hipStreamSynchronize(s));
        }
        g->view.cell_start = g->d_cell_start;
        g->view.pts = g->d_pts;
    }
    if (d_part) (void)hipFree(d_part);
    if (d_cell_of) (void)hipFree(d_cell_of);
    if (d_cursor) (void)hipFree(d_cursor);
    *out_grid = g;
    return UAVQP_OK;
fail:
    if (d_part) (void)hipFree(d_part);
    if (d_cell_of) (void)hipFree(d_cell_of);
    if (d_cursor) (void)hipFree(d_cursor);
    (void)uavqp_obstacle_grid_destroy(nullptr, g);
    return rc;
#undef UAVQP_GRID_HIP
}

// (d_tmax_bits: the pipeline's form -- dt = [the double whose bits are *d_tmax_bits] / (n_samples - 1), formed by the kernel, and
// d_first_hit already holds n_samples: the host neither waits for the longest duration nor launches the fill)
static int ellipsoid_check_grid_impl(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                     const double* d_times, const double* d_coeff, int n_samples, double t0, double dt,
                                     const unsigned long long* d_tmax_bits, const uavqp_grid* grid, double robot_r, double robot_h,
                                     int32_t* d_first_hit, uint8_t* d_flags);
extern "C" int uavqp_ellipsoid_check_grid_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                                 const double* d_times, const double* d_coeff, int n_samples, double t0, double dt,
                                                 const uavqp_grid* grid, double robot_r, double robot_h, int32_t* d_first_hit,
                                                 uint8_t* d_flags) {
    return ellipsoid_check_grid_impl(ctx, r, n_traj, uniform_segments, d_seg_offsets, d_times, d_coeff, n_samples, t0, dt, nullptr, grid, robot_r,
                                     robot_h, d_first_hit, d_flags);
}
static int ellipsoid_check_grid_impl(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                     const double* d_times, const double* d_coeff, int n_samples, double t0, double dt,
                                     const unsigned long long* d_tmax_bits, const uavqp_grid* grid, double robot_r, double robot_h,
                                     int32_t* d_first_hit, uint8_t* d_flags) {
    if (!ctx || !grid || (r != 3 && r != 4) || n_traj < 0 || n_samples < 0 || uniform_segments < 0 || !(robot_r > 0.0) || !(robot_h > 0.0))
        return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0) return UAVQP_OK;
    if (!d_times || !d_coeff || !d_first_hit || (uniform_segments == 0 && !d_seg_offsets) || grid->device != ctx->device)
        return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    if (!d_tmax_bits) hipLaunchKernelGGL(uavqp::fill_i32_kernel, dim3((n_traj + 255) / 256), dim3(256), 0, ctx->stream, d_first_hit, n_traj, (int32_t)n_samples);
    if (n_samples == 0) return UAVQP_OK;
    uavqp::EllipsoidGridArgs a;
    a.tmax_bits = d_tmax_bits;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.n_samples = n_samples;
    a.seg_offsets = d_seg_offsets; a.times = d_times; a.coeff = d_coeff; a.grid = grid->view;
    a.t0 = t0; a.dt = dt; a.robot_r = robot_r; a.robot_h = robot_h; a.first_hit = d_first_hit; a.flags = d_flags;
    const long long total = (long long)n_traj * n_samples;
    long long grid_dim = (total + 63) / 64;                    // one wave per workgroup (the wave pools its candidates through LDS)
    if (grid_dim > (long long)ctx->num_cus * 64) grid_dim = (long long)ctx->num_cus * 64;
    if (r == 3)
        hipLaunchKernelGGL(uavqp::ellipsoid_grid_kernel<3>, dim3((unsigned)grid_dim), dim3(64), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::ellipsoid_grid_kernel<4>, dim3((unsigned)grid_dim), dim3(64), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

extern "C" int uavqp_corridor_from_cloud_device(uavqp_ctx* ctx, int r, int n_traj, int uniform_segments, const int32_t* d_seg_offsets,
                                                int n_rows, const double* d_waypoints, const double* d_times, const double* d_coeff,
                                                const double* d_obstacles, int n_obs, double robot_r, double robot_h, double h_max,
                                                double* d_corr_lo, double* d_corr_hi, double* d_clearance) {
    if (!ctx || (r != 3 && r != 4) || n_traj < 0 || n_rows < 0 || uniform_segments < 0 || n_obs < 0 || !(robot_r > 0.0) ||
        !(robot_h > 0.0) || !(h_max >= 0.0))
        return UAVQP_ERR_INVALID_ARG;
    if (n_traj == 0 || n_rows == 0) return UAVQP_OK;
    if (!d_waypoints || !d_corr_lo || !d_corr_hi || (n_obs > 0 && !d_obstacles) || (uniform_segments == 0 && !d_seg_offsets) ||
        (d_coeff && !d_times) || (uniform_segments > 0 && (long long)n_traj * (uniform_segments + 1) != n_rows))
        return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    uavqp::CloudCorridorArgs a;
    a.n_traj = n_traj; a.uniform = uniform_segments; a.n_rows = n_rows; a.n_obs = n_obs;
    a.seg_offsets = d_seg_offsets; a.waypoints = d_waypoints; a.times = d_times; a.coeff = d_coeff; a.obs = d_obstacles;
    a.robot_r = robot_r; a.robot_h = robot_h; a.h_max = h_max; a.lo = d_corr_lo; a.hi = d_corr_hi; a.clearance = d_clearance;
    long long grid = ((long long)n_rows + 255) / 256;
    if (grid > (long long)ctx->num_cus * 16) grid = (long long)ctx->num_cus * 16;
    a.sort = nullptr; a.row_perm = nullptr; a.row_start = nullptr; a.pt_start = nullptr; a.pts_sorted = nullptr; a.reach = 0.0;
    // Large clouds, boxes only: rows and points sorted along the cloud's longest axis, every block scans the points within `reach`
    // of its rows (obstacle_grid.h, cloud_window_kernel) -- identical boxes, fewer pairs.  The clearance output needs the exhaustive min.
    const bool windowed = !d_clearance && n_obs >= 4096 && n_rows >= 4096 && ctx->settings.cloud_window != 0;
#ifdef UAVQP_EXPERIMENTS
    if (windowed && ctx->settings.cloud_window >= 3) {
        // Round 5, two passes on the 2-D cell grid (cloud_grid2d.h): the rows the bounding box does not cull scan the ring next to them; the ones whose
        // clearance so far does not bound what farther points could change are re-sorted by the radius it implies and scan exactly that -- identical boxes.
        const double rmax = robot_r > robot_h ? robot_r : robot_h, rmin = robot_r > robot_h ? robot_h : robot_r;
        a.reach = rmax * (1.0 + 3.0 * h_max / rmin) * (1.0 + 1e-9) + 1e-9;
        const size_t b_h = sizeof(int32_t) * (uavqp::CLOUD2D_MAX_CELLS + 2), b_h2 = align256(sizeof(int32_t) * ((size_t)uavqp::CLOUD2D_BUCKETS * uavqp::CLOUD2D_MAX_CELLS + 2));
        const size_t b_perm = sizeof(int32_t) * (size_t)n_rows;
        Carve c;
        const int i_cg = c.add(256), i_pstart = c.add(b_h), i_pcur = c.add(b_h), i_rstart = c.add(b_h), i_rcur = c.add(b_h);
        const int i_hist2 = c.add(b_h2), i_cur2 = c.add(b_h2), i_pts = c.add(sizeof(double) * 3 * (size_t)n_obs);
        const int i_perm = c.add(b_perm), i_rbin = c.add(b_perm), i_rkey = c.add(b_perm), i_perm2 = c.add(b_perm), i_rm = c.add(sizeof(double) * (size_t)n_rows);
        const int rc = carve_on(ctx->stream, ctx->ws, c);
        if (rc != UAVQP_OK) return rc;
        uavqp::Cloud2D* d_cg = c.at<uavqp::Cloud2D>(i_cg);
        int32_t *d_pstart = c.at<int32_t>(i_pstart), *d_pcur = c.at<int32_t>(i_pcur), *d_rstart = c.at<int32_t>(i_rstart), *d_rcur = c.at<int32_t>(i_rcur);
        int32_t *d_hist2 = c.at<int32_t>(i_hist2), *d_cur2 = c.at<int32_t>(i_cur2);
        double* d_pts = c.at<double>(i_pts);
        int32_t *d_perm = c.at<int32_t>(i_perm), *d_rbin = c.at<int32_t>(i_rbin), *d_rkey = c.at<int32_t>(i_rkey), *d_perm2 = c.at<int32_t>(i_perm2);
        double* d_rm = c.at<double>(i_rm);
        long long sgrid = ((long long)n_obs + n_rows + 511) / 512;
        if (sgrid > (long long)ctx->num_cus * 2) sgrid = (long long)ctx->num_cus * 2;
        UAVQP_HIP(hipMemsetAsync(d_hist2, 0, b_h2, ctx->stream));
        hipLaunchKernelGGL(uavqp::cloud2d_setup_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_obstacles, n_obs, a.reach / 8.0, d_cg, d_pstart, d_rstart);
        if (r == 3) hipLaunchKernelGGL(uavqp::cloud2d_hist_cull_kernel<3>, dim3((unsigned)sgrid), dim3(256), 0, ctx->stream, a, (const uavqp::Cloud2D*)d_cg, d_pstart, d_rstart, d_rbin);
        else hipLaunchKernelGGL(uavqp::cloud2d_hist_cull_kernel<4>, dim3((unsigned)sgrid), dim3(256), 0, ctx->stream, a, (const uavqp::Cloud2D*)d_cg, d_pstart, d_rstart, d_rbin);
        hipLaunchKernelGGL(uavqp::cloud2d_scan_n_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uavqp::Cloud2D*)d_cg, 1, 1, d_pstart, d_pcur, d_rstart, d_rcur);
        hipLaunchKernelGGL(uavqp::cloud2d_scatter_bin_kernel, dim3((unsigned)sgrid), dim3(256), 0, ctx->stream, d_obstacles, n_obs, (const int32_t*)d_rbin, n_rows,
                           (const uavqp::Cloud2D*)d_cg, d_pcur, d_rcur, d_pts, d_perm);
        a.row_perm = d_perm; a.pt_start = d_pstart; a.pts_sorted = d_pts;
        uavqp::Cloud2PArgs pa;
        pa.c = a; pa.grid = d_cg; pa.row_start = d_rstart; pa.row_key = d_rkey; pa.row_m = d_rm; pa.hist2 = d_hist2; pa.perm2 = d_perm2;
        if (r == 3) hipLaunchKernelGGL(uavqp::cloud2d_pass1_kernel<3>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, pa);
        else hipLaunchKernelGGL(uavqp::cloud2d_pass1_kernel<4>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, pa);
        hipLaunchKernelGGL(uavqp::cloud2d_scan_n_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uavqp::Cloud2D*)d_cg, 0, uavqp::CLOUD2D_BUCKETS, (int32_t*)nullptr,
                           (int32_t*)nullptr, d_hist2, d_cur2);
        long long g2 = ((long long)n_rows + 255) / 256;
        if (g2 > (long long)ctx->num_cus * 8) g2 = (long long)ctx->num_cus * 8;
        hipLaunchKernelGGL(uavqp::cloud2d_scatter2_kernel, dim3((unsigned)g2), dim3(256), 0, ctx->stream, (const int32_t*)d_rkey, n_rows, d_cur2, d_perm2);
        if (r == 3) hipLaunchKernelGGL(uavqp::cloud2d_pass2_kernel<3>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, pa);
        else hipLaunchKernelGGL(uavqp::cloud2d_pass2_kernel<4>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, pa);
    } else if (windowed && ctx->settings.cloud_window == 2) {
        // Round 5: points and rows sorted by the cell of a 2-D grid; a block scans the cells around its rows nearest first and stops as soon
        // as the clearance found bounds what farther points could still change (cloud_grid2d.h) -- identical boxes, a fraction of the pairs.
        const double rmax = robot_r > robot_h ? robot_r : robot_h, rmin = robot_r > robot_h ? robot_h : robot_r;
        a.reach = rmax * (1.0 + 3.0 * h_max / rmin) * (1.0 + 1e-9) + 1e-9;
        const size_t b_h = sizeof(int32_t) * (uavqp::CLOUD2D_MAX_CELLS + 1);
        Carve c;
        const int i_cg = c.add(256), i_pstart = c.add(b_h), i_pcur = c.add(b_h), i_rstart = c.add(b_h), i_rcur = c.add(b_h);
        const int i_pts = c.add(sizeof(double) * 3 * (size_t)n_obs), i_perm = c.add(sizeof(int32_t) * (size_t)n_rows);
        const int rc = carve_on(ctx->stream, ctx->ws, c);
        if (rc != UAVQP_OK) return rc;
        uavqp::Cloud2D* d_cg = c.at<uavqp::Cloud2D>(i_cg);
        unsigned int* d_phase = (unsigned int*)((char*)d_cg + 128);   // (probe builds: blocks per ring, in the grid record's slot)
        int32_t *d_pstart = c.at<int32_t>(i_pstart), *d_pcur = c.at<int32_t>(i_pcur), *d_rstart = c.at<int32_t>(i_rstart), *d_rcur = c.at<int32_t>(i_rcur);
        double* d_pts = c.at<double>(i_pts);
        int32_t* d_perm = c.at<int32_t>(i_perm);
        long long sgrid = ((long long)n_obs + n_rows + 511) / 512;
        if (sgrid > (long long)ctx->num_cus * 2) sgrid = (long long)ctx->num_cus * 2;
#ifdef UAVQP_CLOUD_STATS
        UAVQP_HIP(hipMemsetAsync(d_phase, 0, 16, ctx->stream));
#endif
        hipLaunchKernelGGL(uavqp::cloud2d_setup_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_obstacles, n_obs, a.reach / 8.0, d_cg, d_pstart, d_rstart);
        hipLaunchKernelGGL(uavqp::cloud2d_hist_kernel, dim3((unsigned)sgrid), dim3(256), 0, ctx->stream, d_obstacles, n_obs, d_waypoints, n_rows,
                           (const uavqp::Cloud2D*)d_cg, d_pstart, d_rstart);
        hipLaunchKernelGGL(uavqp::cloud2d_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uavqp::Cloud2D*)d_cg, d_pstart, d_pcur, d_rstart, d_rcur);
        hipLaunchKernelGGL(uavqp::cloud2d_scatter_kernel, dim3((unsigned)sgrid), dim3(256), 0, ctx->stream, d_obstacles, n_obs, d_waypoints, n_rows,
                           (const uavqp::Cloud2D*)d_cg, d_pcur, d_rcur, d_pts, d_perm);
        a.row_perm = d_perm; a.pt_start = d_pstart; a.pts_sorted = d_pts;
        uavqp::Cloud2DArgs ga;
        ga.c = a; ga.grid = d_cg; ga.phase_count = nullptr;
#ifdef UAVQP_CLOUD_STATS
        ga.phase_count = d_phase;      // probe build (tools/cloud_phase_probe.py): blocks per ring
        ctx->dbg_queue = d_phase;
#else
        (void)d_phase;
#endif
        if (r == 3)
            hipLaunchKernelGGL(uavqp::cloud_grid2d_kernel<3>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, ga);
        else
            hipLaunchKernelGGL(uavqp::cloud_grid2d_kernel<4>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, ga);
    } else
#endif
    if (windowed) {
        const double rmax = robot_r > robot_h ? robot_r : robot_h, rmin = robot_r > robot_h ? robot_h : robot_r;
        a.reach = rmax * (1.0 + 3.0 * h_max / rmin) * (1.0 + 1e-9) + 1e-9;
        const size_t b_ph = sizeof(int32_t) * (uavqp::CLOUD_PT_BINS + 1), b_rh = sizeof(int32_t) * (uavqp::CLOUD_ROW_BINS + 2), b_perm = sizeof(int32_t) * (size_t)n_rows;
        Carve c;
        const int i_cs = c.add(256), i_pstart = c.add(b_ph), i_pcur = c.add(b_ph), i_rstart = c.add(b_rh), i_rcur = c.add(b_rh);
        const int i_pts = c.add(sizeof(double) * 3 * (size_t)n_obs), i_perm = c.add(b_perm), i_rbin = c.add(b_perm);
        const int rc = carve_on(ctx->stream, ctx->ws, c);
        if (rc != UAVQP_OK) return rc;
        uavqp::CloudSort* d_cs = c.at<uavqp::CloudSort>(i_cs);
        int32_t *d_pstart = c.at<int32_t>(i_pstart), *d_pcur = c.at<int32_t>(i_pcur), *d_rstart = c.at<int32_t>(i_rstart), *d_rcur = c.at<int32_t>(i_rcur);
        double* d_pts = c.at<double>(i_pts);
        int32_t *d_perm = c.at<int32_t>(i_perm), *d_rbin = c.at<int32_t>(i_rbin);
        long long sgrid = ((long long)n_obs + n_rows + 511) / 512;   // every block: one contiguous slice of the keys, bins counted in LDS
        if (sgrid > (long long)ctx->num_cus * 2) sgrid = (long long)ctx->num_cus * 2;
        hipLaunchKernelGGL(uavqp::cloud_sort_setup_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_obstacles, n_obs, a.reach, d_cs, d_pstart, d_rstart);
        // (the histogram pass also computes every row's attitude: rows the cloud's bounding box proves capped go to an extra bin and are never scanned)
        if (r == 3) hipLaunchKernelGGL(uavqp::cloud_sort_hist_kernel<3>, dim3((unsigned)sgrid), dim3(256), 0, ctx->stream, a, (const uavqp::CloudSort*)d_cs, d_pstart, d_rstart, d_rbin);
        else hipLaunchKernelGGL(uavqp::cloud_sort_hist_kernel<4>, dim3((unsigned)sgrid), dim3(256), 0, ctx->stream, a, (const uavqp::CloudSort*)d_cs, d_pstart, d_rstart, d_rbin);
        hipLaunchKernelGGL(uavqp::cloud_sort_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_pstart, d_pcur, d_rstart, d_rcur);
        hipLaunchKernelGGL(uavqp::cloud_sort_scatter_kernel, dim3((unsigned)sgrid), dim3(256), 0, ctx->stream, d_obstacles, n_obs, (const int32_t*)d_rbin, n_rows,
                           (const uavqp::CloudSort*)d_cs, d_pcur, d_rcur, d_pts, d_perm);
        a.sort = d_cs; a.row_perm = d_perm; a.row_start = d_rstart; a.pt_start = d_pstart; a.pts_sorted = d_pts;
        long long wgrid = ((long long)n_rows + 127) / 128;        // 128 rows per block: two waves share a row and split the points (four: no further gain)
        if (wgrid > (long long)ctx->num_cus * 24) wgrid = (long long)ctx->num_cus * 24;
        if (r == 3)
            hipLaunchKernelGGL((uavqp::cloud_window_kernel<3, 2>), dim3((unsigned)wgrid), dim3(256), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL((uavqp::cloud_window_kernel<4, 2>), dim3((unsigned)wgrid), dim3(256), 0, ctx->stream, a);
    } else if (r == 3)
        hipLaunchKernelGGL(uavqp::cloud_corridor_kernel<3>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(uavqp::cloud_corridor_kernel<4>, dim3((unsigned)grid), dim3(256), 0, ctx->stream, a);
    UAVQP_HIP(hipGetLastError());
    return UAVQP_OK;
}

// ===================================================================================================
// BASELINE config 5 as one call
// ===================================================================================================
#include "uavqp_pipeline.h"

// ===================================================================================================
// Cost, exact time gradient and the duration optimiser
// ===================================================================================================
#include "uavqp_time_opt.h"

// ===================================================================================================
// Backward pass of the equality-constrained solve
// ===================================================================================================
#include "uavqp_adjoint.h"

// ===================================================================================================
// Velocity / acceleration limit penalty and the limit-aware duration optimiser
// ===================================================================================================
#include "uavqp_limits.h"

// ===================================================================================================
// Attitude penalty: specific thrust, tilt and body rate of the vehicle that flies the trajectory
// ===================================================================================================
#include "uavqp_attitude.h"

// ===================================================================================================
// Moving-obstacle penalty: a trajectory against tracks that are not the batch's to move
// ===================================================================================================
#include "uavqp_moving.h"
#include "uavqp_moving_cert.h"   // the certificate against the same tracks: bounds where the penalty samples

// ===================================================================================================
// Certified continuous-time bounds (Bernstein enclosure) of solved trajectories and the verdict against limits
// ===================================================================================================
#include "uavqp_envelope.h"

// ===================================================================================================
// Signed distance field of an occupancy grid and the clearance penalty
// ===================================================================================================
#include "uavqp_esdf.h"

// ===================================================================================================
// Certified continuous-time clearance of solved trajectories against the distance field (needs the map of uavqp_esdf.h)
// ===================================================================================================
#include "uavqp_clearance_cert.h"

// ===================================================================================================
// Waypoint gradient of the control cost and the waypoint optimiser against the distance field
// ===================================================================================================
#include "uavqp_waypoint_opt.h"

// ===================================================================================================
// Fused flight penalty (limits + clearance) and the joint optimiser of waypoints and durations
// ===================================================================================================
#include "uavqp_spacetime.h"
#include "uavqp_spacetime_lbfgs.h"

// ===================================================================================================
// Separation penalty between the vehicles of a swarm on a shared clock
// ===================================================================================================
#include "uavqp_swarm.h"
#include "uavqp_swarm_opt.h"

// ===================================================================================================
// Certified continuous-time separation between the vehicles of a swarm (shares the swarm penalty's description of the swarms)
// ===================================================================================================
#include "uavqp_separation_cert.h"

// ===================================================================================================
// N3: quadrotor_msgs/PolynomialTrajectory packer (host only)
// ===================================================================================================
extern "C" int uavqp_pack_polynomial_trajectory(int r, int n_seg, const double* coeff_traj, const double* times, double* coef_x,
                                                double* coef_y, double* coef_z, double* time_out, uint32_t* order_out,
                                                uint32_t* num_order_out, uint32_t* num_segment_out) {
    if ((r != 3 && r != 4) || n_seg < 1 || !coeff_traj || !times || !coef_x || !coef_y || !coef_z || !time_out) return UAVQP_ERR_INVALID_ARG;
    for (int i = 0; i < n_seg; ++i)
        if (!(times[i] > 0.0) || !(times[i] < INFINITY)) return UAVQP_ERR_INVALID_ARG;
    const size_t per_axis = (size_t)n_seg * 2 * r;
    // each axis slice of the solver output IS the message's per-axis array: coef[i * (num_order + 1) + j] multiplies t^j in segment i
    // (poly_traj_server.cpp:68-78 reads exactly that index)
    std::memcpy(coef_x, coeff_traj, sizeof(double) * per_axis);
    std::memcpy(coef_y, coeff_traj + per_axis, sizeof(double) * per_axis);
    std::memcpy(coef_z, coeff_traj + 2 * per_axis, sizeof(double) * per_axis);
    std::memcpy(time_out, times, sizeof(double) * (size_t)n_seg);
    if (order_out)
        for (int i = 0; i < n_seg; ++i) order_out[i] = (uint32_t)(2 * r - 1);
    if (num_order_out) *num_order_out = (uint32_t)(2 * r - 1);
    if (num_segment_out) *num_segment_out = (uint32_t)n_seg;
    return UAVQP_OK;
}

// ===================================================================================================
// Multi-GPU entry points (uavqp_comm.h)
// ===================================================================================================
extern "C" int uavqp_shard_bounds(int n_traj, int world, int32_t* bounds) {
    if (n_traj < 0 || world < 1 || !bounds) return UAVQP_ERR_INVALID_ARG;
    for (int g = 0; g <= world; ++g) bounds[g] = (int32_t)(((long long)n_traj * g) / world);
    return UAVQP_OK;
}

extern "C" int uavqp_shard_bounds_ragged(const int32_t* seg_offsets, int n_traj, int world, int32_t* bounds) {
    if (n_traj < 0 || world < 1 || !bounds || !seg_offsets) return UAVQP_ERR_INVALID_ARG;
    for (int b = 0; b < n_traj; ++b)
        if (seg_offsets[b + 1] < seg_offsets[b]) return UAVQP_ERR_INVALID_ARG;
    const long long total = (long long)seg_offsets[n_traj] - seg_offsets[0];
    bounds[0] = 0;
    for (int g = 1; g < world; ++g) {
        // first trajectory whose offset reaches g / world of the segments (exact integer comparison: off * world >= total * g)
        const long long want = total * g;
        const int32_t* lo = seg_offsets + bounds[g - 1];
        const int32_t* hi = seg_offsets + n_traj;
        const int32_t* it = std::lower_bound(lo, hi, want, [&](int32_t off, long long w) { return ((long long)off - seg_offsets[0]) * world < w; });
        bounds[g] = (int32_t)(it - seg_offsets);
    }
    bounds[world] = n_traj;
    return UAVQP_OK;
}

#define UAVQP_RCCL(expr)                                                                             \
    do {                                                                                             \
        ncclResult_t r_ = (expr);                                                                    \
        if (r_ != ncclSuccess) {                                                                     \
            g_last_error = std::string(#expr) + ": " + uavqp::rccl().GetErrorString(r_);             \
            return UAVQP_ERR_RCCL;                                                                   \
        }                                                                                            \
    } while (0)

static int rccl_ready() {
    if (!uavqp::rccl().load()) {
        g_last_error = uavqp::rccl().error;
        return UAVQP_ERR_RCCL;
    }
    return UAVQP_OK;
}

extern "C" int uavqp_comm_unique_id(void* id_out) {
    static_assert(UAVQP_UNIQUE_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "token size follows RCCL");
    if (!id_out) return UAVQP_ERR_INVALID_ARG;
    int rc = rccl_ready();
    if (rc != UAVQP_OK) return rc;
    ncclUniqueId id;
    UAVQP_RCCL(uavqp::rccl().GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return UAVQP_OK;
}

extern "C" int uavqp_comm_create(uavqp_ctx* ctx, int rank, int world, const void* unique_id) {
    if (!ctx || !unique_id || world < 1 || rank < 0 || rank >= world) return UAVQP_ERR_INVALID_ARG;
    if (ctx->comm.comm) { g_last_error = "this ctx already owns a communicator"; return UAVQP_ERR_INVALID_ARG; }
    int rc = rccl_ready();
    if (rc != UAVQP_OK) return rc;
    UAVQP_HIP(hipSetDevice(ctx->device));
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    ncclComm_t comm = nullptr;
    UAVQP_RCCL(uavqp::rccl().CommInitRank(&comm, world, id, rank));
    ctx->comm.comm = comm;
    ctx->comm.rank = rank;
    ctx->comm.world = world;
    return UAVQP_OK;
}

extern "C" int uavqp_comm_info(const uavqp_ctx* ctx, int32_t* rank_out, int32_t* world_out) {
    if (!ctx || (!rank_out && !world_out)) return UAVQP_ERR_INVALID_ARG;
    if (!ctx->comm.comm) { g_last_error = "no communicator: call uavqp_comm_create first"; return UAVQP_ERR_INVALID_ARG; }
    // asked of RCCL, not remembered: ncclCommUserRank / ncclCommCount of the communicator the ctx owns
    int rk = -1, wd = -1;
    UAVQP_RCCL(uavqp::rccl().CommUserRank(ctx->comm.comm, &rk));
    UAVQP_RCCL(uavqp::rccl().CommCount(ctx->comm.comm, &wd));
    if (rank_out) *rank_out = rk;
    if (world_out) *world_out = wd;
    return UAVQP_OK;
}

extern "C" int uavqp_comm_destroy(uavqp_ctx* ctx) {
    if (!ctx) return UAVQP_ERR_INVALID_ARG;
    if (!ctx->comm.comm) return UAVQP_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ncclComm_t c = ctx->comm.comm;
    ctx->comm = uavqp::Comm();
    UAVQP_RCCL(uavqp::rccl().CommDestroy(c));
    return UAVQP_OK;
}

template <typename T>
static int allgather_shards(uavqp_ctx* ctx, const T* d_local, const int64_t* counts, T* d_full, ncclDataType_t dt) {
    if (!ctx || !counts || !d_full) return UAVQP_ERR_INVALID_ARG;
    if (!ctx->comm.comm) { g_last_error = "no communicator: call uavqp_comm_create first"; return UAVQP_ERR_INVALID_ARG; }
    const int world = ctx->comm.world, rank = ctx->comm.rank;
    bool equal = true;
    int64_t total = 0;
    for (int g = 0; g < world; ++g) {
        if (counts[g] < 0) return UAVQP_ERR_INVALID_ARG;
        equal = equal && counts[g] == counts[0];
        total += counts[g];
    }
    if (total == 0) return UAVQP_OK;
    if (counts[rank] > 0 && !d_local) return UAVQP_ERR_INVALID_ARG;
    UAVQP_HIP(hipSetDevice(ctx->device));
    uavqp::RcclApi& R = uavqp::rccl();
    if (equal) {
        UAVQP_RCCL(R.AllGather(d_local, d_full, (size_t)counts[0], dt, ctx->comm.comm, ctx->stream));
        return UAVQP_OK;
    }
    // all-gather-v: every rank sends its shard to every peer directly, one hop per peer on the xGMI full mesh
    std::vector<int64_t> off(world + 1, 0);
    for (int g = 0; g < world; ++g) off[g + 1] = off[g] + counts[g];
    UAVQP_RCCL(R.GroupStart());
    ncclResult_t first_err = ncclSuccess;
    const char* what = "";
    for (int g = 0; g < world && first_err == ncclSuccess; ++g) {
        if (g == rank) continue;
        if (counts[rank] > 0) {
            first_err = R.Send(d_local, (size_t)counts[rank], dt, g, ctx->comm.comm, ctx->stream);
            what = "ncclSend";
        }
        if (first_err == ncclSuccess && counts[g] > 0) {
            first_err = R.Recv(d_full + off[g], (size_t)counts[g], dt, g, ctx->comm.comm, ctx->stream);
            what = "ncclRecv";
        }
    }
    // the group is closed on EVERY path: an open group would swallow the next collective of this thread
    const ncclResult_t end_err = R.GroupEnd();
    if (first_err != ncclSuccess) {
        g_last_error = std::string(what) + ": " + R.GetErrorString(first_err);
        return UAVQP_ERR_RCCL;
    }
    if (end_err != ncclSuccess) {
        g_last_error = std::string("ncclGroupEnd: ") + R.GetErrorString(end_err);
        return UAVQP_ERR_RCCL;
    }
    if (counts[rank] > 0 && d_local != d_full + off[rank])
        UAVQP_HIP(hipMemcpyAsync(d_full + off[rank], d_local, sizeof(T) * (size_t)counts[rank], hipMemcpyDeviceToDevice, ctx->stream));
    return UAVQP_OK;
}

extern "C" int uavqp_allgather_coeffs(uavqp_ctx* ctx, const double* d_local, const int64_t* counts, double* d_full) {
    return allgather_shards<double>(ctx, d_local, counts, d_full, ncclFloat64);
}

extern "C" int uavqp_allgather_status(uavqp_ctx* ctx, const int32_t* d_local, const int64_t* counts, int32_t* d_full) {
    return allgather_shards<int32_t>(ctx, d_local, counts, d_full, ncclInt32);
}
