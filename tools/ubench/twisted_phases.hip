// Per-wave timeline of the twisted kernel + back-to-back launch timing.  Debug tool.
//   -DTILE_=4|8|16|32 -DLPT_=16|8|2|2   tile shape          -DONE_=1   the one-whole-tile-per-wave instantiation (tiles 4 and 8)
//   -DNO_STAMPS                         the product kernel untouched: launch timing only
// The kernel is the product's, with the product's argument list (csrc/Makefile: unit-flags -> kernarg preload).  Its UAVQP_STAMP points are
// taken over: every wave reads the cycle counter into SCALAR REGISTERS -- at entry, before it has needed any argument; when its input loads
// are issued; when they have landed; behind the meeting knot; at its end -- and stores the lot once, at its end, through a pointer held in a
// __device__ variable (fetched there, not at entry).  "entry -> loads issued" and "entry -> loaded" per wave say what stands in front of the loads.
// ONE_ builds: the kernel never reads its batch size, so the host passes (grid + k) * TILE_ in it and launch k of a back-to-back run stamps
// into slab k: "last end -> next entry" is the time between the last wave's end of one launch and the first wave's entry of the next on the
// 100 MHz counter -- the drain of the stores plus the launch boundary.  The same kernel is then timed in a captured chain of 20.
//   -DUAVQP_TIMING_BUILD -DUAVQP_TW_DROP_STORES   (qp_twisted.h) every coefficient store gets the out-of-range offset: what the store path costs
#include <hip/hip_runtime.h>
#ifndef TILE_
#define TILE_ 32
#endif
#ifndef LPT_
#define LPT_ 2
#endif
#ifndef ONE_
#define ONE_ 0
#endif
#ifndef NO_STAMPS
#define TL_WORDS 8
#define TL_SLABS 8
__device__ long long* g_timeline;   // [grid][TL_WORDS]
#define UAVQP_STAMP(i) UAVQP_STAMP_##i
#define UAVQP_STAMP_5 const long long tl_real0 = __builtin_amdgcn_s_memrealtime(), tl_entry = __builtin_readcyclecounter();
// (sched_barrier: the scheduler may not move the arithmetic that follows a stamp in front of it)
#define UAVQP_STAMP_6 __builtin_amdgcn_sched_barrier(0); const long long tl_issued = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0);
#define UAVQP_STAMP_0 __builtin_amdgcn_sched_barrier(0); const long long tl_loaded = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0);
#define UAVQP_STAMP_1
#define UAVQP_STAMP_2
#define UAVQP_STAMP_3 const long long tl_met = __builtin_readcyclecounter();
#define UAVQP_STAMP_4                                                                                               \
    if (tile == (int)blockIdx.x) { /* the wave's first tile */                                                      \
        const long long tl_end = __builtin_readcyclecounter(), tl_real1 = __builtin_amdgcn_s_memrealtime();         \
        if (threadIdx.x == 0) {                                                                                     \
            const int tl_slab = ONE_ ? a.n_traj / TILE_ - (int)gridDim.x : 0;                                       \
            long long* tl_p = g_timeline + ((size_t)tl_slab * gridDim.x + blockIdx.x) * TL_WORDS;                   \
            tl_p[0] = tl_real0; tl_p[1] = tl_entry; tl_p[2] = tl_issued; tl_p[3] = tl_loaded; tl_p[4] = tl_met;     \
            tl_p[5] = tl_end; tl_p[6] = tl_real1;                                                                   \
        }                                                                                                           \
    }
#endif
#include "../../uav_motion_planning_amd/csrc/uavqp.hip"
#include <algorithm>
#include <random>
#include <vector>

__global__ void empty_kernel(int* p) { if (p && threadIdx.x == 1234567) *p = 1; }

static void row(const char* name, std::vector<double> v) {
    std::sort(v.begin(), v.end());
    double sum = 0;
    for (double x : v) sum += x;
    const size_t n = v.size();
    printf("  %-22s min %8.0f  p50 %8.0f  p90 %8.0f  max %8.0f  mean %8.0f\n", name, v[0], v[n / 2], v[(n * 9) / 10], v[n - 1], sum / n);
}

int main(int argc, char** argv) {
    const int B = argc > 1 ? atoi(argv[1]) : 4096, M = 8, r = 4;
    const int n_tiles = (B + TILE_ - 1) / TILE_, grid = n_tiles < 1024 ? n_tiles : 1024;
    if (ONE_ && (B % TILE_ != 0 || grid != n_tiles)) { printf("ONE_: the batch must be whole tiles, no more of them than 1024 waves\n"); return 2; }
    std::mt19937_64 g(1);
    std::uniform_real_distribution<double> u(-2, 2), ut(0.5, 2.0);
    std::vector<double> wp((size_t)B * (M + 1) * 3), T((size_t)B * M), bc((size_t)B * 2 * (r - 1) * 3, 0.0);
    for (auto& x : wp) x = u(g);
    for (auto& x : T) x = ut(g);
    double *dwp, *dT, *dbc, *dout; int* dst;
    hipMalloc(&dwp, wp.size() * 8); hipMalloc(&dT, T.size() * 8); hipMalloc(&dbc, bc.size() * 8);
    hipMalloc(&dout, (size_t)B * 3 * M * 2 * r * 8); hipMalloc(&dst, B * 4);
    hipMemcpy(dwp, wp.data(), wp.size() * 8, hipMemcpyHostToDevice);
    hipMemcpy(dT, T.data(), T.size() * 8, hipMemcpyHostToDevice);
    hipMemcpy(dbc, bc.data(), bc.size() * 8, hipMemcpyHostToDevice);
    uavqp::BatchArgs a{};
    a.n_traj = B; a.uniform = M; a.max_segments = M; a.waypoints = dwp; a.times = dT; a.bc = dbc; a.coeff = dout; a.status = dst;
    uavqp::TwistedParams tp(a);   // the library's own marshalling
    const void* fn = (const void*)&uavqp::solve_twisted_kernel<4, 8, TILE_, LPT_, ONE_ != 0>;
    hipStream_t s; if (getenv("NB")) hipStreamCreateWithFlags(&s, hipStreamNonBlocking); else hipStreamCreate(&s);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    printf("solve_twisted_kernel<4, 8, %d, %d, %s>  B = %d  grid = %d\n", TILE_, LPT_, ONE_ ? "true" : "false", B, grid);
#ifndef NO_STAMPS
    long long* dtl;
    hipMalloc(&dtl, (size_t)TL_SLABS * grid * TL_WORDS * 8);
    hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), &dtl, sizeof(dtl));
    std::vector<long long> tl((size_t)grid * TL_WORDS);
    for (int rep = 0; rep < 4; ++rep) {
        hipMemset(dtl, 0, tl.size() * 8);
        if (hipLaunchKernel(fn, dim3(grid), dim3(64), tp.ptr, 0, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { printf("launch failed\n"); return 1; }
        hipMemcpy(tl.data(), dtl, tl.size() * 8, hipMemcpyDeviceToHost);
        long long first = tl[0], last = tl[6];
        for (int w = 0; w < grid; ++w) { first = std::min(first, tl[(size_t)w * TL_WORDS]); last = std::max(last, tl[(size_t)w * TL_WORDS + 6]); }
        std::vector<double> entry, end_, issued, loaded, met, total;
        for (int w = 0; w < grid; ++w) {
            const long long* p = &tl[(size_t)w * TL_WORDS];
            entry.push_back((p[0] - first) * 10.0); end_.push_back((p[6] - first) * 10.0);   // 100 MHz counter -> ns
            issued.push_back(double(p[2] - p[1])); loaded.push_back(double(p[3] - p[1])); met.push_back(double(p[4] - p[1])); total.push_back(double(p[5] - p[1]));
        }
        printf("launch %d: timeline over %d waves (cycles from the wave's entry; ns of the 100 MHz counter from the first wave's entry)\n", rep, grid);
        row("entry ns", entry);
        row("entry -> issued cyc", issued);
        row("entry -> loaded cyc", loaded);
        row("entry -> met cyc", met);
        row("entry -> end cyc", total);
        row("end ns", end_);
        printf("  first entry -> last end: %lld ns\n", (last - first) * 10);
    }
#if ONE_
    // TL_SLABS launches back to back, each into its own slab (the batch size argument carries the slab: see the head of this file)
    for (int rep = 0; rep < 3; ++rep) {
        std::vector<long long> tls((size_t)TL_SLABS * grid * TL_WORDS);
        hipMemset(dtl, 0, tls.size() * 8);
        hipStreamSynchronize(s);
        for (int k = 0; k < TL_SLABS; ++k) {
            uavqp::BatchArgs ak = a;
            ak.n_traj = (grid + k) * TILE_;
            uavqp::TwistedParams tpk(ak);   // (the arguments are copied at the launch)
            if (hipLaunchKernel(fn, dim3(grid), dim3(64), tpk.ptr, 0, s) != hipSuccess) { printf("launch failed\n"); return 1; }
        }
        if (hipStreamSynchronize(s) != hipSuccess) { printf("launch failed\n"); return 1; }
        hipMemcpy(tls.data(), dtl, tls.size() * 8, hipMemcpyDeviceToHost);
        long long fe[TL_SLABS], le[TL_SLABS];
        for (int k = 0; k < TL_SLABS; ++k) {
            const long long* q = &tls[(size_t)k * grid * TL_WORDS];
            fe[k] = q[0]; le[k] = q[6];
            for (int w = 0; w < grid; ++w) { fe[k] = std::min(fe[k], q[(size_t)w * TL_WORDS]); le[k] = std::max(le[k], q[(size_t)w * TL_WORDS + 6]); }
        }
        printf("back-to-back %d, launches 1..%d: last end -> next entry ns:", rep, TL_SLABS - 1);
        for (int k = 0; k + 1 < TL_SLABS; ++k) printf(" %lld", (fe[k + 1] - le[k]) * 10);
        printf("   | first entry -> last end ns:");
        for (int k = 0; k < TL_SLABS; ++k) printf(" %lld", (le[k] - fe[k]) * 10);
        printf("   | entry -> next entry ns:");
        for (int k = 0; k + 1 < TL_SLABS; ++k) printf(" %lld", (fe[k + 1] - fe[k]) * 10);
        printf("\n");
    }
#endif
#endif
    const int K = 200;
    for (int rep = 0; rep < 3; ++rep) {
        hipEventRecord(e0, s);
        for (int i = 0; i < K; ++i) hipLaunchKernel(fn, dim3(grid), dim3(64), tp.ptr, 0, s);
        hipEventRecord(e1, s); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        printf("twisted<4,8> B=%d: %.2f us/launch back-to-back\n", B, ms * 1e3 / K);
    }
    {
        // the same launch in a captured chain of 20, replayed
        const int CH = 20, REPLAYS = 50;
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        bool okc = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess;
        for (int i = 0; okc && i < CH; ++i) okc = hipLaunchKernel(fn, dim3(grid), dim3(64), tp.ptr, 0, s) == hipSuccess;
        okc = hipStreamEndCapture(s, &graph) == hipSuccess && okc;
        okc = okc && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (!okc) { printf("capture failed\n"); return 1; }
        for (int i = 0; i < 5; ++i) hipGraphLaunch(exec, s);
        hipStreamSynchronize(s);
        for (int rep = 0; rep < 3; ++rep) {
            hipEventRecord(e0, s);
            for (int i = 0; i < REPLAYS; ++i) hipGraphLaunch(exec, s);
            hipEventRecord(e1, s); hipEventSynchronize(e1);
            float msc; hipEventElapsedTime(&msc, e0, e1);
            printf("twisted<4,8> B=%d: %.2f us/launch in a captured chain of %d (%d replays)\n", B, msc * 1e3 / (REPLAYS * CH), CH, REPLAYS);
        }
        for (int rep = 0; rep < 3; ++rep) {   // one replay at a time, as a step loop that waits for each chain does
            double sum = 0;
            for (int i = 0; i < REPLAYS; ++i) {
                hipEventRecord(e0, s);
                hipGraphLaunch(exec, s);
                hipEventRecord(e1, s); hipEventSynchronize(e1);
                float msc; hipEventElapsedTime(&msc, e0, e1);
                sum += msc;
            }
            printf("twisted<4,8> B=%d: %.2f us/launch in a captured chain of %d, one replay per wait\n", B, sum * 1e3 / (REPLAYS * CH), CH);
        }
        hipGraphExecDestroy(exec); hipGraphDestroy(graph);
    }
    hipEventRecord(e0, s);
    for (int i = 0; i < K; ++i) hipLaunchKernelGGL(empty_kernel, dim3(grid), dim3(64), 0, s, (int*)nullptr);
    hipEventRecord(e1, s); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("empty kernel grid=%d: %.2f us/launch back-to-back\n", grid, ms * 1e3 / K);
    return 0;
}
