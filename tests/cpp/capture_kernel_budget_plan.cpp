// What uavqp_capture_end makes of a capture under any setting of the two fuse knobs, from the host rules alone
// (uav_motion_planning_amd/csrc/uavqp_capture.h: lay_out, group_cap -- the function rebuild_captured asks -- and fuse_groups with one cap
// per node; kernel_instances.h: which shapes have a group kernel and an eight-per-wave kernel), without the HIP runtime:
// tests/test_gpu_capture_kernel_budget.py hands this program the solves it captured and reads back which of them share a launch.
// (capture_fuse_waves_plan.cpp is the same with one budget for every kernel, capture_fuse_plan.cpp with a named count.)
// stdin:  "lanes nodes_per_lane fuse budget num_cus count" -- fuse and budget as UAVQP_CAPTURE_FUSE and UAVQP_CAPTURE_FUSE_WAVES have
//         them, "-" = not set -- then per solve "r M tile n_traj waypoints times bc coeff status" (addresses, 0 = none)
// stdout: one line per launch of the replay, "stage lane cap node node ..." (cap: that of the launch's first solve)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernel_instances.h"
#include "uavqp_capture.h"

using namespace uavqp_capture;

int main() {
    int lanes = 0, per_lane = 0, num_cus = 0, count = 0;
    char fuse_text[32], budget_text[32];
    if (std::scanf("%d %d %31s %31s %d %d", &lanes, &per_lane, fuse_text, budget_text, &num_cus, &count) != 6 || count < 0 || count > (int)NODES_MAX) return 2;
    const int fuse_named = fuse_named_from_env(std::strcmp(fuse_text, "-") == 0 ? nullptr : fuse_text);
    const int waves_named = fuse_waves_named_from_env(std::strcmp(budget_text, "-") == 0 ? nullptr : budget_text);
    std::vector<Record> rec;
    std::vector<Shape> shape;
    std::vector<int> cap;
    for (int k = 0; k < count; ++k) {
        int r = 0, M = 0, tile = 0, n_traj = 0;
        unsigned long long p[5];
        if (std::scanf("%d %d %d %d %llu %llu %llu %llu %llu", &r, &M, &tile, &n_traj, &p[0], &p[1], &p[2], &p[3], &p[4]) != 9) return 2;
        if (tile < 1 || n_traj < 1 || M < 1 || r < 1) return 2;
        // the extents and the launch shape of uavqp_solve_batch_device (uavqp.hip: capture_note, the tile rule)
        const size_t n = (size_t)n_traj, tot = n * (size_t)M;
        Record x;
        x.read[0] = range_of((const void*)(uintptr_t)p[0], sizeof(double) * 3 * (tot + n));
        x.read[1] = range_of((const void*)(uintptr_t)p[1], sizeof(double) * tot);
        x.read[2] = range_of((const void*)(uintptr_t)p[2], sizeof(double) * n * 2 * (size_t)(r - 1) * 3);
        x.coeff = range_of((const void*)(uintptr_t)p[3], sizeof(double) * 3 * 2 * (size_t)r * tot);
        x.status = range_of((const void*)(uintptr_t)p[4], sizeof(int32_t) * n);
        rec.push_back(x);
        const int n_tiles = (n_traj + tile - 1) / tile, max_wg = num_cus * 4;
        Shape s;
        s.fn = (const void*)(uintptr_t)(r * 10000 + M * 100 + tile);   // one kernel function per (r, M, tile)
        s.grid = (unsigned)(n_tiles < max_wg ? n_tiles : max_wg);
        s.block = 64;
        s.n_traj = n_traj;
        s.one = (int)s.grid == n_tiles && n_traj % tile == 0 && uavqp_twisted_group_exists(r, M, tile);
        shape.push_back(s);
        cap.push_back(group_cap(fuse_named, waves_named, tile, s.one, n_traj, s.grid, s.one && tile == 4 && uavqp_twisted_group8_exists(r, M)));
    }
    const std::vector<char> dead = dead_status_stores(rec);
    const Fused f = fuse_groups(rec, dead, lay_out(rec, dead, lanes), shape, cap, lanes, per_lane);
    for (size_t s = 0; s < f.group.size(); ++s)
        for (size_t l = 0; l < f.group[s].size(); ++l)
            for (const std::vector<int>& g : f.group[s][l]) {
                std::printf("%d %d %d", (int)s, (int)l, cap[(size_t)g[0]]);
                for (int k : g) std::printf(" %d", k);
                std::printf("\n");
            }
    return 0;
}
