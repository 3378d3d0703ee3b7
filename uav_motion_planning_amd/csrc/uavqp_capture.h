// uavqp_capture.h -- which captured solves may run side by side when their graph is replayed, and in which lane each of them goes: the
// dependency analysis and the lane layout behind uavqp_capture_end (uavqp.hip).  A stream capture orders every launch behind the one
// before it; steps of a launch-bound inner loop usually touch disjoint buffers, and about 30 % of each is the GPU idling at that kernel
// boundary (docs/measurement_log.md 5.1, 6, 7).  The replay is laid out by lay_out: a solve follows the solve it conflicts with into that
// solve's lane, so a rotation over any number of buffer sets is ONE stage of chains.  analyse / stage_starts are the layout before it
// (lane of node k: k % lanes), kept with their results as the reference the conflict rules are pinned against.
// fuse_groups then cuts every lane into groups of independent solves of one shape, each replayed as ONE launch.
// Host-only: byte ranges and indices, no HIP type -- compiles without the runtime (tests/cpp/test_capture_deps.cpp, test_capture_lanes.cpp,
// test_capture_fuse.cpp, test_capture_fuse_waves.cpp, test_capture_kernel_budget.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace uavqp_capture {

// bytes [lo, hi) of the address space; lo == hi is "nothing".  Two ranges that touch end to start do not overlap.
struct Range {
    uintptr_t lo = 0, hi = 0;
    bool empty() const { return hi <= lo; }
    bool overlaps(const Range& o) const { return !empty() && !o.empty() && lo < o.hi && o.lo < hi; }
    bool covers(const Range& o) const { return !empty() && !o.empty() && lo <= o.lo && o.hi <= hi; }
};
static inline Range range_of(const void* p, size_t bytes) {
    Range g;
    if (p && bytes) { g.lo = (uintptr_t)p; g.hi = g.lo + bytes; }
    return g;
}

// What one captured launch touches.  A launch whose extents the host does not know (ragged batches), or that goes through a workspace
// of the ctx, is a barrier: it conflicts with everything before and after it.
struct Record {
    bool barrier = false;
    Range read[3];    // waypoints, durations, boundary values
    Range coeff;      // written
    Range status;     // written; empty when the caller passed no status array
};

struct Plan {
    std::vector<std::vector<int>> preds;   // per node: the nodes it waits for (transitive reduction, descending)
    std::vector<char> status_dead;         // per node: a later node overwrites every status it would store before anything reads one
    bool parallel = false;                 // at least two nodes are mutually independent
};

static constexpr int LANES_DEFAULT = 4;    // what bench.py's `pipelined` sub-record was measured with; HIP's default hardware-queue count
static constexpr int LANES_MAX = 8;
static constexpr size_t NODES_MAX = 4096;  // the ancestor sets are n^2 / 8 bytes: larger captures stay the chain they were captured as

// UAVQP_CAPTURE_LANES (1..8, anything else: the default) and GPU_MAX_HW_QUEUES as found in the environment (either may be null).  A process
// given fewer than 4 hardware queues replays its graphs as captured: parallel branches want a queue each.
static inline int lanes_from_env(const char* lanes_env, const char* hw_queues_env) {
    int lanes = LANES_DEFAULT;
    if (lanes_env && *lanes_env) {
        const int v = std::atoi(lanes_env);
        if (v >= 1 && v <= LANES_MAX) lanes = v;
    }
    if (hw_queues_env && *hw_queues_env && std::atoi(hw_queues_env) < 4) lanes = 1;
    return lanes;
}

static inline bool writes_into(const Record& w, bool w_status_dead, const Range& g) {
    return w.coeff.overlaps(g) || (!w_status_dead && w.status.overlaps(g));
}
static inline bool touches(const Record& x, const Range& g) {   // any read or write of x, its status store included
    return x.read[0].overlaps(g) || x.read[1].overlaps(g) || x.read[2].overlaps(g) || x.coeff.overlaps(g) || x.status.overlaps(g);
}
// must k (later) wait for i (earlier)?  read-after-write, write-after-read, write-after-write; a dead status store is no write
static inline bool conflict(const Record& i, bool i_dead, const Record& k, bool k_dead) {
    if (i.barrier || k.barrier) return true;
    for (int q = 0; q < 3; ++q)
        if (writes_into(i, i_dead, k.read[q]) || writes_into(k, k_dead, i.read[q])) return true;
    if (writes_into(i, i_dead, k.coeff)) return true;
    return !k_dead && writes_into(i, i_dead, k.status);
}

// The status store of node i is dead when the NEXT node that touches its range at all is a solve whose status range covers it and that
// touches it in no other way: nothing captured reads a status, so when the graph completes the array holds the last writer's values, as
// in serial order.  Anything else -- a partial overlap, a read of those bytes, a barrier in between -- keeps the store (and its edge).
static inline std::vector<char> dead_status_stores(const std::vector<Record>& rec) {
    const size_t n = rec.size();
    std::vector<char> dead(n, 0);
    for (size_t i = 0; i < n; ++i) {
        if (rec[i].barrier || rec[i].status.empty()) continue;
        const Range& s = rec[i].status;
        for (size_t k = i + 1; k < n; ++k) {
            if (rec[k].barrier) break;
            if (!touches(rec[k], s)) continue;
            const Record& x = rec[k];
            dead[i] = x.status.covers(s) && !x.coeff.overlaps(s) && !x.read[0].overlaps(s) && !x.read[1].overlaps(s) && !x.read[2].overlaps(s);
            break;
        }
    }
    return dead;
}

// Edges of the rebuilt graph: conflicts + the lane edges k - lanes -> k (at most `lanes` chains run side by side), transitively reduced.
// Nodes are in capture order, so every edge points forward and node k's ancestors are known once k - 1 .. 0 have been looked at,
// nearest first: a candidate already among the ancestors is implied by an edge taken before it.
static inline Plan analyse(const std::vector<Record>& rec, int lanes) {
    const size_t n = rec.size();
    Plan plan;
    plan.preds.assign(n, std::vector<int>());
    if (n > NODES_MAX) lanes = 1;
    if (lanes < 1) lanes = 1;
    plan.status_dead = lanes > 1 ? dead_status_stores(rec) : std::vector<char>(n, 0);
    if (lanes == 1) {    // the captured chain
        for (size_t k = 1; k < n; ++k) plan.preds[k].push_back((int)k - 1);
        return plan;
    }
    const size_t words = (n + 63) / 64;
    std::vector<uint64_t> anc(n * words, 0);    // anc[k]: bit i = node i runs before node k
    for (size_t k = 0; k < n; ++k) {
        uint64_t* mine = &anc[k * words];
        size_t n_anc = 0;
        for (size_t i = k; i-- > 0;) {
            if (mine[i / 64] >> (i % 64) & 1) { ++n_anc; continue; }
            if (i + (size_t)lanes != k && !conflict(rec[i], plan.status_dead[i] != 0, rec[k], plan.status_dead[k] != 0)) continue;
            plan.preds[k].push_back((int)i);
            const uint64_t* theirs = &anc[i * words];
            for (size_t w = 0; w <= i / 64; ++w) mine[w] |= theirs[w];
            mine[i / 64] |= (uint64_t)1 << (i % 64);
            ++n_anc;
        }
        if (n_anc < k) plan.parallel = true;
    }
    return plan;
}

// How the plan is replayed: node k belongs to lane k % lanes, each lane of a stage is one chain graph on a stream of its own, and a
// stage ends where the lanes have to meet -- in front of a node that waits for a node of ANOTHER lane of the same stage (a path between
// two lanes of a stage contains such an edge, so edges the reduction dropped need no look).  Returns the first node of every stage.
static inline std::vector<int> stage_starts(const Plan& plan, int lanes) {
    std::vector<int> starts;
    const int n = (int)plan.preds.size();
    if (lanes < 1) lanes = 1;
    for (int k = 0; k < n; ++k) {
        bool cut = k == 0;
        for (int i : plan.preds[k])
            if (!cut && i >= starts.back() && i % lanes != k % lanes) cut = true;
        if (cut) starts.push_back(k);
    }
    return starts;
}

// How many lanes a stage of `nodes` launches is replayed on.  Every lane beyond the first is one more graph launch and a fork / join
// through events: 10-16 us of host time per replay, where a solve that no longer waits at a kernel boundary gains about 1.3 us
// (docs/measurement_log.md: 20 captured steps on 4 lanes replay SLOWER than the chain, 35-step stages gain on 2 lanes and not on 4).
// A lane pays for itself after about 10 launches; it is used when the stage has 16 for it.  Lane of node k: (k % lanes) % that many --
// a stage has no conflict between two classes k % lanes, so they may share a lane in any combination.
// UAVQP_CAPTURE_LANE_NODES (1..4096) overrides the 16: 1 puts every stage on as many lanes as it has launches for (tests, A/B runs).
static constexpr int NODES_PER_LANE_MIN = 16;
static inline int lane_nodes_from_env(const char* env) {
    const int v = env && *env ? std::atoi(env) : 0;
    return v >= 1 && v <= (int)NODES_MAX ? v : NODES_PER_LANE_MIN;
}
static inline int lanes_that_pay(int nodes, int lanes, int nodes_per_lane = NODES_PER_LANE_MIN) {
    const int by_size = nodes / (nodes_per_lane < 1 ? 1 : nodes_per_lane);
    return by_size < 1 ? 1 : (by_size < lanes ? by_size : lanes);
}

// The layout a capture is replayed with: the lane of every node, the first node of every stage, and whether any stage has two busy lanes.
// In capture order, with s the first node of the current stage and P the lanes of the nodes of [s, k) that node k conflicts with:
//   P empty     node k takes the least-loaded lane of the stage (ties: the lowest index), so the lanes of a stage fill from lane 0 up;
//   P one lane  node k takes it and follows its predecessor in that lane's chain -- the only ordering a stage provides;
//   P more      the lanes have to meet: a new stage starts at k, in lane 0.
// A barrier is a stage of its own.  More than NODES_MAX nodes, or one lane: one stage, everything in lane 0.
// Hence: two conflicting nodes are in different stages (ordered by the join) or in the same lane (ordered by the chain).  Lanes may be
// merged afterwards in any combination (lane % w): that only adds order.  `status_dead` is dead_status_stores(rec), or all zero.
// The scan is one conflict test per earlier node of the stage; a node's hull (every byte it reads or writes, a dead status store left
// out) rejects most pairs in two comparisons, so 4096 nodes stay in the milliseconds.
struct Layout {
    std::vector<int> lane, starts;
    bool parallel = false;
};
static inline Layout lay_out(const std::vector<Record>& rec, const std::vector<char>& status_dead, int lanes) {
    const int n = (int)rec.size();
    Layout out;
    out.lane.assign((size_t)n, 0);
    if (n == 0) return out;
    if ((size_t)n > NODES_MAX || lanes <= 1 || status_dead.size() != (size_t)n) {
        out.starts.push_back(0);
        return out;
    }
    if (lanes > LANES_MAX) lanes = LANES_MAX;
    std::vector<Range> hull((size_t)n);
    for (int k = 0; k < n; ++k) {
        Range h;
        h.lo = UINTPTR_MAX;
        const Range* part[5] = {&rec[k].read[0], &rec[k].read[1], &rec[k].read[2], &rec[k].coeff, &rec[k].status};
        for (int q = 0; q < (status_dead[k] ? 4 : 5); ++q) {
            if (part[q]->empty()) continue;
            if (part[q]->lo < h.lo) h.lo = part[q]->lo;
            if (part[q]->hi > h.hi) h.hi = part[q]->hi;
        }
        hull[k] = h;
    }
    int load[LANES_MAX] = {};
    int s = 0;
    bool fresh = true;   // the next node starts a stage
    for (int k = 0; k < n; ++k) {
        unsigned met = 0;    // bit l: node k conflicts with a node of lane l of this stage
        bool cut = fresh || rec[k].barrier;
        for (int i = s; !cut && i < k; ++i) {
            if (!hull[i].overlaps(hull[k]) || !conflict(rec[i], status_dead[i] != 0, rec[k], status_dead[k] != 0)) continue;
            met |= 1u << out.lane[i];
            cut = (met & (met - 1)) != 0;
        }
        if (cut) {
            out.starts.push_back(k);
            s = k;
            for (int l = 0; l < lanes; ++l) load[l] = 0;
            load[0] = 1;
            fresh = rec[k].barrier;
            continue;
        }
        int lane = 0;
        if (met) {
            while (!(met >> lane & 1)) ++lane;
        } else {
            for (int l = 1; l < lanes; ++l)
                if (load[l] < load[lane]) lane = l;
        }
        out.lane[k] = lane;
        ++load[lane];
        if (lane != 0) out.parallel = true;   // lane 0 holds the first node of the stage
    }
    return out;
}

// The lanes of a replay when UAVQP_CAPTURE_LANES does not name a count: 2, the ctx stream and ONE stream of the ctx's own.  A lane gains
// only where its stream has a hardware queue to itself, and HIP neither says nor lets a caller choose which queue a stream gets.  Measured
// (docs/measurement_log.md, 2026-10-18): the ctx stream and the first lane stream had a queue each in every kind of process; in a plain
// process the second and third shared those two queues (a kernel trace shows the four streams on two queues, in pairs), so 4 lanes
// replayed no faster than 2, while in a process whose communication library had created streams first they did not share and 4 lanes were
// 10 % faster -- a replay whose speed depends on what else the process did before.  Two lanes replay alike in both.  A count that
// UAVQP_CAPTURE_LANES names is taken as it is (lanes_from_env), and fewer than 4 hardware queues keep the chain either way.
static constexpr int REPLAY_LANES_DEFAULT = 2;
static inline int replay_lanes_from_env(const char* lanes_env, const char* hw_queues_env) {
    const int lanes = lanes_from_env(lanes_env, hw_queues_env);
    const int asked = lanes_env && *lanes_env ? std::atoi(lanes_env) : 0;
    if (asked >= 1 && asked <= LANES_MAX) return lanes;
    return lanes < REPLAY_LANES_DEFAULT ? lanes : REPLAY_LANES_DEFAULT;
}

// ---- Groups: independent solves of one shape that follow each other in a lane are replayed as ONE launch (qp_twisted.h:
// solve_twisted_group_kernel, grid (n_tiles, members)).  A replayed small-batch solve is bound by its launch -- the kernel boundary and the
// dispatch ramp of its grid cost more than its waves live (docs/measurement_log.md, 2026-10-20) -- so a lane pays one boundary per group
// instead of one per solve, and the waves of several members share a SIMD (at least three of the eight-per-wave kernel: qp_twisted.h).  fuse_groups runs AFTER lay_out and changes nothing of it.
//
// What a launch is, as far as grouping goes: two launches with equal keys run the same kernel over grids of the same shape.
struct Shape {
    const void* fn = nullptr;                  // the kernel function of the launch
    unsigned grid = 0, block = 0, lds_bytes = 0;
    int n_traj = 0;
    bool one = false;                          // grid == n_tiles and n_traj % TILE == 0: the launch takes the one-tile-per-wave instantiation
};
static inline bool same_shape(const Shape& a, const Shape& b) {
    return a.fn == b.fn && a.grid == b.grid && a.block == b.block && a.lds_bytes == b.lds_bytes && a.n_traj == b.n_traj && a.one == b.one;
}
// UAVQP_CAPTURE_FUSE (1..8): the most solves one launch of a replay carries, for every group; 1 = every solve its own launch.
// Not set (or anything else): the cap of a group follows from a BUDGET OF WAVES per launch, UAVQP_CAPTURE_FUSE_WAVES (a positive
// integer, for every kernel; anything else: the default of the kernel the group will run -- FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT for the
// eight-per-wave kernel, FUSE_WAVES_DEFAULT for every other: fuse_budget), and from the waves one member adds in that kernel (member_waves):
//   fuse_cap = min(FUSE_MAX, max(FUSE_DEFAULT, budget / waves per member)).
// Why waves and not solves.  More members per launch replay faster at 200 and at 20 steps, but launches of 4096 and 8192 waves from two
// lanes compete for the wave slots, and then a two-lane replay depends on which hardware queues the runtime gave the two streams: with
// the four-per-wave group kernel a process that had initialised its communication library first replayed 4-5 % (4 members, 4096 waves)
// and 5-8 % (8 members, 8192 waves) faster than a plain one, with 2 members (2048 waves) 0.5 % -- and a default whose speed depends on
// what else the process did was ruled out when the lane count was chosen (REPLAY_LANES_DEFAULT; tests/test_gpu_bench_two_ranks.py holds
// the two kinds of process within 6 % of each other).  That finding is about the size of a launch; a count of solves stands for it only
// while every kernel puts as many trajectories in a wave.  The eight-per-wave kernel (group_kernel_choice) halves the waves of a solve:
// two of its members are 1024 waves, one per SIMD, and a lone wave has nothing to issue during its own load wait and LDS round trips.
// FUSE_DEFAULT, the cap before there was a budget, remains as the lower bound: no shape gets fewer members than it had.
// FUSE_WAVES_DEFAULT is 2048 waves, chosen on MI355X between 4096 and 2048 by plain / communication-library / plain triples of the
// benchmark (docs/measurement_log.md, 2026-10-21; the process with the library against the faster plain run): at 4096 the headline
// shape (8 members of the eight-per-wave kernel, 512 waves each) stayed inside +4 % (+0.1 .. +3.5 %), but a batch of 4092 -- no whole
// number of eights, 4 members of the 16-lane group kernel at 1023 waves each -- replayed 5.8-6.4 % faster with the library; at 2048 the
// headline shape has 4 members (-2.6 .. +0.3 %) and the batch of 4092 the 2 it had.
static constexpr int FUSE_MAX = 8;             // == uavqp::GROUP_MAX (qp_twisted.h): the pointer sets one kernarg struct holds
static constexpr int FUSE_DEFAULT = 2;
static constexpr int FUSE_WAVES_DEFAULT = 2048;
// The eight-per-wave kernel has a default budget of its own, used where UAVQP_CAPTURE_FUSE_WAVES names none (fuse_budget): the
// placement dependence that holds FUSE_WAVES_DEFAULT at 2048 was the 16-lane group kernel's.  Measured on MI355X among 2048, 3072 and
// 4096 on the kernel that fits three waves per SIMD, it stays 2048: all three were inside the plain / communication-library / plain
// bound, 4096 was 2 % ahead on the headline shape (less than the run-to-run range) and made 4096 x (r = 3, M = 16) 8-18 % slower.
// Triples, runs and the shapes taken apart: docs/measurement_log.md, 2026-10-21, the entry on three waves per SIMD.
static constexpr int FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT = 2048;
static inline int fuse_from_env(const char* env) {
    const int v = env && *env ? std::atoi(env) : 0;
    return v >= 1 && v <= FUSE_MAX ? v : FUSE_DEFAULT;
}
// The count UAVQP_CAPTURE_FUSE names (1..8, what fuse_from_env returns for it), or 0 where it names none and the budget decides.
static inline int fuse_named_from_env(const char* env) {
    const int v = env && *env ? std::atoi(env) : 0;
    return v >= 1 && v <= FUSE_MAX ? v : 0;
}
// The budget UAVQP_CAPTURE_FUSE_WAVES names (a positive integer that fits an int, nothing before or behind it), or 0 where it names
// none and every kernel has the default of its own (fuse_budget, below).
static inline int fuse_waves_named_from_env(const char* env) {
    if (!env || !*env) return 0;
    char* end = nullptr;
    const long long v = std::strtoll(env, &end, 10);   // (saturates on overflow: out of range below)
    return *end == '\0' && env[0] >= '0' && env[0] <= '9' && v >= 1 && v <= 2147483647LL ? (int)v : 0;
}
static inline int fuse_waves_from_env(const char* env) {
    const int v = fuse_waves_named_from_env(env);
    return v ? v : FUSE_WAVES_DEFAULT;
}
static inline int fuse_cap(int budget, int waves_per_member) {
    if (budget <= 0 || waves_per_member <= 0) return FUSE_DEFAULT;
    const int fit = budget / waves_per_member;
    return fit < FUSE_DEFAULT ? FUSE_DEFAULT : (fit > FUSE_MAX ? FUSE_MAX : fit);
}
// The replay as it is built: stage s runs on width[s] lanes (lanes_that_pay; node k in lane lay.lane[k] % width[s]), and
// group[s][l] holds the nodes of lane l of stage s, in capture order, cut into groups -- one launch each.  In capture order a node joins the
// OPEN (the last) group of its lane only if
//   * it is no barrier and takes the one-tile-per-wave instantiation (Shape::one),
//   * its shape key equals the group's,
//   * it conflicts with NO member of the group (conflict(), with the dead-status flags lay_out was given),
//   * the group has fewer than F members -- with one cap per node (`cap`, cut to FUSE_MAX): fewer than the cap of its FIRST member.
//     (rebuild_captured derives a node's cap from its shape, and equal shape keys are equal n_traj, grid and kernel function: one
//     group, one cap);
// otherwise it opens a new group.  Hence
//   * every node is in exactly one group;
//   * the groups of a lane are in capture order: every node of a group comes before every node of the next one;
//   * the members of a group are pairwise conflict-free, so their relative order is free -- they may run side by side;
//   * two conflicting nodes are in different stages, or in one lane in different groups in capture order: ordered as before.
// F <= 1 gives every node a group of its own: the chains of lay_out.  One comparison per member of the open group: at most F - 1 per node.
struct Fused {
    std::vector<int> width;                                            // per stage
    std::vector<std::vector<std::vector<std::vector<int>>>> group;     // [stage][lane][group][member] -> node
    bool side_by_side = false;                                         // some stage has two busy lanes
    bool fused = false;                                                // some group has two members
};
static inline Fused fuse_groups(const std::vector<Record>& rec, const std::vector<char>& status_dead, const Layout& lay, const std::vector<Shape>& shape,
                                const std::vector<int>& cap, int lanes, int nodes_per_lane = NODES_PER_LANE_MIN) {
    Fused out;
    const int n = (int)rec.size();
    if (n == 0 || lay.lane.size() != (size_t)n || lay.starts.empty() || shape.size() != (size_t)n || cap.size() != (size_t)n) return out;
    if (lanes < 1) lanes = 1;
    const bool have_dead = status_dead.size() == (size_t)n;
    for (size_t s = 0; s < lay.starts.size(); ++s) {
        const int first = lay.starts[s], last = s + 1 < lay.starts.size() ? lay.starts[s + 1] : n;
        const int width = lanes_that_pay(last - first, lanes, nodes_per_lane);
        out.width.push_back(width);
        out.group.emplace_back((size_t)width);
        for (int k = first; k < last; ++k) {
            std::vector<std::vector<int>>& chain = out.group.back()[(size_t)(lay.lane[k] % width)];
            const bool k_dead = have_dead && status_dead[k] != 0;
            const int F = chain.empty() ? 0 : (cap[(size_t)chain.back()[0]] < FUSE_MAX ? cap[(size_t)chain.back()[0]] : FUSE_MAX);
            bool join = !chain.empty() && !rec[k].barrier && shape[k].one && (int)chain.back().size() < F && same_shape(shape[chain.back()[0]], shape[k]);
            if (join)    // (the first member of a group that takes a second is no barrier and `one`: same_shape compares the flag)
                for (int i : chain.back())
                    if (rec[i].barrier || conflict(rec[i], have_dead && status_dead[i] != 0, rec[k], k_dead)) { join = false; break; }
            if (!join) chain.emplace_back();
            chain.back().push_back(k);
            if (chain.back().size() > 1) out.fused = true;
        }
        int busy = 0;
        for (const auto& chain : out.group.back()) busy += !chain.empty();
        if (busy > 1) out.side_by_side = true;
    }
    return out;
}
// One cap F for every node (UAVQP_CAPTURE_FUSE names a count; the CPU programs under tests/cpp).
static inline Fused fuse_groups(const std::vector<Record>& rec, const std::vector<char>& status_dead, const Layout& lay, const std::vector<Shape>& shape,
                                int F, int lanes, int nodes_per_lane = NODES_PER_LANE_MIN) {
    return fuse_groups(rec, status_dead, lay, shape, std::vector<int>(rec.size(), F), lanes, nodes_per_lane);
}

// Which kernel the node of a group gets (uavqp.hip: rebuild_captured).  A group of two or more launches of the 16-lane one-tile-per-wave
// kernel (tile 4) whose batch is a whole number of eights takes the eight-trajectories-per-wave kernel of its shape, where there is one
// (qp_twisted.h: solve_twisted_group8_kernel -- the 16-lane arithmetic without the elimination two lane pairs repeat); every other group
// of two or more takes the group kernel of its launches' own tile; a group of one is the launch as it was captured.
//   members      solves in the group (fuse_groups)
//   tile         trajectories per wave of the captured launches (4, 8, ...)
//   one          the launches take the one-tile-per-wave instantiation and their shape has a group kernel at that tile (Shape::one)
//   has_group8   the shape has a solve_twisted_group8_kernel (kernel_instances.h: uavqp_twisted_group8_exists)
enum GroupKernel { GROUP_AS_CAPTURED = 0, GROUP_OWN_TILE = 1, GROUP_EIGHT_PER_WAVE = 2 };
static inline GroupKernel group_kernel_choice(int members, int tile, bool one, int n_traj, bool has_group8) {
    if (members < 2 || !one) return GROUP_AS_CAPTURED;   // (fuse_groups never gives a launch without `one` a second member)
    if (tile == 4 && has_group8 && n_traj > 0 && n_traj % 8 == 0) return GROUP_EIGHT_PER_WAVE;
    return GROUP_OWN_TILE;
}
// The waves ONE member adds to a group launch, in the kernel a group of launches of this shape runs: the eight-per-wave kernel has a
// wave for every eight trajectories, the group kernel of the launch's own tile the waves of the captured launch (`grid`, block 64).
// A launch that is never fused (not `one`) counts as captured.
static inline int member_waves(int tile, bool one, int n_traj, unsigned grid, bool has_group8) {
    return group_kernel_choice(FUSE_DEFAULT, tile, one, n_traj, has_group8) == GROUP_EIGHT_PER_WAVE ? n_traj / 8 : (int)grid;
}

// The budget of waves a group of launches of this shape is cut by: the one UAVQP_CAPTURE_FUSE_WAVES names (`waves_named` > 0:
// fuse_waves_named_from_env), for every kernel; where it names none, the default of the kernel the group runs.
static inline int fuse_budget(int waves_named, int tile, bool one, int n_traj, bool has_group8) {
    if (waves_named > 0) return waves_named;
    return group_kernel_choice(FUSE_DEFAULT, tile, one, n_traj, has_group8) == GROUP_EIGHT_PER_WAVE ? FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT : FUSE_WAVES_DEFAULT;
}
// The cap of a group whose first member is a launch of this shape, as rebuild_captured gives it to fuse_groups: the count
// UAVQP_CAPTURE_FUSE names (`fuse_named` 1..8) overrides everything; otherwise the budget over the waves of a member.
static inline int group_cap(int fuse_named, int waves_named, int tile, bool one, int n_traj, unsigned grid, bool has_group8) {
    if (fuse_named >= 1) return fuse_named < FUSE_MAX ? fuse_named : FUSE_MAX;
    return fuse_cap(fuse_budget(waves_named, tile, one, n_traj, has_group8), member_waves(tile, one, n_traj, grid, has_group8));
}

// The knobs as the process environment has them NOW: read when a capture ends (uavqp_capture_end), never on a launch path.
// fuse_named: the count UAVQP_CAPTURE_FUSE names, 0 where a budget of waves decides (fuse_named_from_env).
// fuse_waves_named: the budget UAVQP_CAPTURE_FUSE_WAVES names, 0 where every kernel has its own default (fuse_waves_named_from_env).
struct Knobs { int lanes, nodes_per_lane, fuse_named, fuse_waves_named; };
static inline Knobs knobs_from_environment() {
    return Knobs{replay_lanes_from_env(std::getenv("UAVQP_CAPTURE_LANES"), std::getenv("GPU_MAX_HW_QUEUES")), lane_nodes_from_env(std::getenv("UAVQP_CAPTURE_LANE_NODES")),
                 fuse_named_from_env(std::getenv("UAVQP_CAPTURE_FUSE")), fuse_waves_named_from_env(std::getenv("UAVQP_CAPTURE_FUSE_WAVES"))};
}

}  // namespace uavqp_capture
