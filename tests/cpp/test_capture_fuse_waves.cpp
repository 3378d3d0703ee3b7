// Host-only test of how many solves a launch of a replay may carry when UAVQP_CAPTURE_FUSE names no count
// (uav_motion_planning_amd/csrc/uavqp_capture.h: fuse_cap, member_waves, fuse_waves_from_env, fuse_named_from_env and the fuse_groups
// overload that takes one cap per node): the cap follows from a budget of waves per launch and from the kernel a group of that shape
// runs.  Without the HIP runtime: the edges of the arithmetic, the two parsers, the waves of a member against group_kernel_choice, the
// per-node overload against the int-F form on 500 random captures, captures whose shapes have DIFFERENT caps against the brute-force
// statement of the grouping rule, and the benchmark's rotation.
// Compiled and run by tests/test_capture_fuse_waves.py, once plain and once under the address and undefined-behaviour sanitizers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "uavqp_capture.h"

using namespace uavqp_capture;

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static Range at(uintptr_t lo, size_t bytes) {
    Range g;
    g.lo = lo;
    g.hi = lo + bytes;
    return g;
}
// solve number `set` of a family with disjoint buffers: 4 KiB apart, inputs in the first 3 KiB, coefficients in the last; no status
static Record solve(int set) {
    const uintptr_t base = 0x100000 + (uintptr_t)set * 0x1000;
    Record x;
    x.read[0] = at(base, 0x400);
    x.read[1] = at(base + 0x400, 0x400);
    x.read[2] = at(base + 0x800, 0x400);
    x.coeff = at(base + 0xC00, 0x400);
    return x;
}
static Record barrier() {
    Record x;
    x.barrier = true;
    return x;
}
static const uintptr_t STATUS = 0x900000;
typedef std::vector<int> Ints;
typedef std::vector<Ints> Chain;   // the groups of one lane

// Two kernel functions, only their addresses count: launches of KERNEL_A have an eight-per-wave kernel for their groups, those of
// KERNEL_B have none (as (4, 8) and a shape outside the group8 list).  All launches are tile 4.
static const int KERNEL_A = 0, KERNEL_B = 0;
static bool has_group8(const Shape& s) { return s.fn == &KERNEL_A; }
static Shape shape_a() {   // 4096 trajectories, one tile of 4 per wave: 1024 waves as captured, 512 in the eight-per-wave kernel
    Shape s;
    s.fn = &KERNEL_A; s.grid = 1024; s.block = 64; s.n_traj = 4096; s.one = true;
    return s;
}
static Shape shape_b() {   // same grid, no eight-per-wave kernel: 1024 waves per member
    Shape s = shape_a();
    s.fn = &KERNEL_B;
    return s;
}
static Shape shape_half() {   // half the batch: 256 waves per member
    Shape s = shape_a();
    s.grid = 512; s.n_traj = 2048;
    return s;
}
static Shape shape_odd() {   // n % 8 != 0: the group kernel of the launch's own tile, 1023 waves per member
    Shape s = shape_a();
    s.grid = 1023; s.n_traj = 4092;
    return s;
}
static Shape shape_ragged() {   // a launch that does not take the one-tile-per-wave instantiation: never fused
    Shape s = shape_a();
    s.n_traj = 4094; s.one = false;
    return s;
}
static int waves_of(const Shape& s) { return member_waves(4, s.one, s.n_traj, s.grid, has_group8(s)); }
static Ints caps_for(const std::vector<Shape>& shape, int budget) {
    Ints cap;
    for (const Shape& s : shape) cap.push_back(fuse_cap(budget, waves_of(s)));
    return cap;
}

static Ints sizes(const Chain& c) {
    Ints out;
    for (const Ints& g : c) out.push_back((int)g.size());
    return out;
}
static int launches(const Fused& f) {
    int c = 0;
    for (const auto& stage : f.group)
        for (const Chain& chain : stage) c += (int)chain.size();
    return c;
}

// ---- random captures: a fixed-seed generator (the one of test_capture_fuse.cpp, restated, with the shape whose batch is no whole
// number of eights among the random shapes); nothing of the functions under test in it
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % below;
}
static void random_capture(std::vector<Record>& rec, std::vector<Shape>& shape) {
    const int sets = 1 + (int)rnd(9), n = 2 + (int)rnd(59);
    const int status_mode = (int)rnd(4);         // 0 none, 1 one shared array, 2 one array per set, 3 views shifted into each other
    const bool rotate = rnd(3) != 0;             // a rotation over the sets, or sets at random
    const bool with_barriers = rnd(4) == 0, with_aliases = rnd(2) == 0;
    const int shape_mode = (int)rnd(3);          // 0 one shape, 1 runs of two shapes, 2 shapes at random (ragged ones among them)
    rec.clear();
    shape.clear();
    Shape run = shape_a();
    for (int k = 0; k < n; ++k) {
        if (with_barriers && rnd(12) == 0) {
            rec.push_back(barrier());
            shape.push_back(Shape());
            continue;
        }
        const int set = rotate ? k % sets : (int)rnd((uint32_t)sets);
        Record x = solve(set);
        if (status_mode == 1) x.status = at(STATUS, 256);
        if (status_mode == 2) x.status = at(STATUS + (uintptr_t)set * 256, 256);
        if (status_mode == 3) x.status = at(STATUS + (uintptr_t)rnd(3) * 64, 256);
        if (with_aliases && rnd(10) == 0) {      // an input read out of another set's coefficients (read-after-write)
            const Record other = solve((int)rnd((uint32_t)sets));
            x.read[rnd(3)] = at(other.coeff.lo + 16 * rnd(8), 0x100);
        }
        if (with_aliases && rnd(14) == 0) {      // coefficients written over another set's input (write-after-read)
            const Record other = solve((int)rnd((uint32_t)sets));
            x.coeff = at(other.read[rnd(3)].lo + 8 * rnd(16), 0x400);
        }
        rec.push_back(x);
        if (shape_mode == 1 && rnd(7) == 0) run = run.fn == &KERNEL_A ? shape_b() : shape_a();
        if (shape_mode == 2) {
            const uint32_t pick = rnd(7);
            run = pick == 0 ? shape_b() : pick == 1 ? shape_half() : pick == 2 ? shape_ragged() : pick == 3 ? shape_odd() : shape_a();
        }
        shape.push_back(run);
    }
}

// The brute-force statement of section "Groups" of uavqp_capture.h, from the layout and the records alone, with "fewer than F members"
// read as "fewer than the cap of the group's first member".  `cf` is conflict() for every pair, worked out once per capture.
static bool holds(const std::vector<Record>& rec, const std::vector<char>& cf, const Layout& lay, const std::vector<Shape>& shape, const Fused& f,
                  const Ints& cap, int lanes, int per_lane) {
    const int n = (int)rec.size();
    auto conflicting = [&](int i, int k) { return cf[(size_t)i * (size_t)n + (size_t)k] != 0; };
    auto room = [&](const Ints& g) { return cap[(size_t)g[0]] < FUSE_MAX ? cap[(size_t)g[0]] : FUSE_MAX; };   // members the group may have
    if (f.group.size() != lay.starts.size() || f.width.size() != lay.starts.size()) return false;
    Ints stage_of((size_t)n, -1), lane_of((size_t)n, -1), group_of((size_t)n, -1), seen((size_t)n, 0);
    bool fused = false, side_by_side = false;
    for (size_t s = 0; s < lay.starts.size(); ++s) {
        const int first = lay.starts[s], last = s + 1 < lay.starts.size() ? lay.starts[s + 1] : n;
        if (f.width[s] != lanes_that_pay(last - first, lanes, per_lane) || (int)f.group[s].size() != f.width[s]) return false;
        int busy = 0;
        for (int l = 0; l < f.width[s]; ++l) {
            const Chain& chain = f.group[s][(size_t)l];
            busy += !chain.empty();
            // the lane's groups, laid end to end, are the lane's nodes in capture order: every node once, groups in capture order
            Ints flat, want;
            for (size_t g = 0; g < chain.size(); ++g) {
                if (chain[g].empty()) return false;
                for (int k : chain[g]) {
                    if (k < 0 || k >= n || seen[(size_t)k]++) return false;
                    flat.push_back(k);
                    stage_of[(size_t)k] = (int)s; lane_of[(size_t)k] = l; group_of[(size_t)k] = (int)g;
                }
                if ((int)chain[g].size() > (room(chain[g]) < 1 ? 1 : room(chain[g]))) return false;
                fused = fused || chain[g].size() > 1;
            }
            for (int k = first; k < last; ++k)
                if (lay.lane[(size_t)k] % f.width[s] == l) want.push_back(k);
            if (flat != want) return false;
            for (size_t g = 0; g < chain.size(); ++g) {
                // members: one shape (hence one cap), the one-tile-per-wave instantiation, no barrier, pairwise conflict-free
                for (size_t x = 0; x < chain[g].size(); ++x)
                    for (size_t y = 0; y < x; ++y) {
                        const int i = chain[g][y], k = chain[g][x];
                        if (rec[(size_t)i].barrier || rec[(size_t)k].barrier || !shape[(size_t)i].one || !shape[(size_t)k].one) return false;
                        if (!same_shape(shape[(size_t)i], shape[(size_t)k]) || cap[(size_t)i] != cap[(size_t)k]) return false;
                        if (conflicting(i, k)) return false;
                    }
                // a group is closed only for a reason: its successor's first node could not have joined it
                if (g + 1 < chain.size()) {
                    const int k = chain[g + 1][0];
                    bool could = !rec[(size_t)k].barrier && shape[(size_t)k].one && (int)chain[g].size() < room(chain[g]);
                    for (int i : chain[g])
                        could = could && !rec[(size_t)i].barrier && same_shape(shape[(size_t)i], shape[(size_t)k]) && !conflicting(i, k);
                    if (could) return false;
                }
            }
        }
        side_by_side = side_by_side || busy > 1;
    }
    for (int k = 0; k < n; ++k)
        if (seen[(size_t)k] != 1) return false;
    // two conflicting nodes: different stages, or one lane and different groups in capture order
    for (int k = 0; k < n; ++k)
        for (int i = 0; i < k; ++i) {
            if (!conflicting(i, k)) continue;
            if (stage_of[(size_t)i] > stage_of[(size_t)k]) return false;
            if (stage_of[(size_t)i] < stage_of[(size_t)k]) continue;
            if (lane_of[(size_t)i] != lane_of[(size_t)k] || group_of[(size_t)i] >= group_of[(size_t)k]) return false;
        }
    return fused == f.fused && side_by_side == f.side_by_side;
}
static std::vector<char> conflicts_of(const std::vector<Record>& rec, const std::vector<char>& dead) {
    const size_t n = rec.size();
    std::vector<char> cf(n * n, 0);
    for (size_t k = 0; k < n; ++k)
        for (size_t i = 0; i < k; ++i) cf[i * n + k] = conflict(rec[i], dead[i] != 0, rec[k], dead[k] != 0);
    return cf;
}

int main() {
    // ---- fuse_cap: min(FUSE_MAX, max(FUSE_DEFAULT, budget / waves))
    CHECK(FUSE_DEFAULT == 2 && FUSE_MAX == 8 && FUSE_WAVES_DEFAULT >= 1);
    CHECK(fuse_cap(4096, 16384) == 2 && fuse_cap(4096, 4097) == 2 && fuse_cap(1, 2) == 2);   // a budget below one member's waves: the lower bound
    CHECK(fuse_cap(4096, 4096) == 2 && fuse_cap(4096, 2048) == 2 && fuse_cap(4096, 2047) == 2);   // one member, two members
    CHECK(fuse_cap(4096, 1366) == 2 && fuse_cap(4096, 1365) == 3 && fuse_cap(4096, 1025) == 3);   // 4096 / 1365 = 3.0007
    CHECK(fuse_cap(4096, 1024) == 4 && fuse_cap(4096, 1023) == 4 && fuse_cap(2048, 1023) == 2 && fuse_cap(2048, 1024) == 2);
    CHECK(fuse_cap(4096, 683) == 5 && fuse_cap(4096, 682) == 6 && fuse_cap(4096, 586) == 6 && fuse_cap(4096, 585) == 7 && fuse_cap(4096, 513) == 7);
    CHECK(fuse_cap(4096, 512) == 8 && fuse_cap(2048, 512) == 4 && fuse_cap(1024, 512) == 2 && fuse_cap(512, 512) == 2);
    CHECK(fuse_cap(4096, 511) == 8 && fuse_cap(4096, 1) == 8 && fuse_cap(2147483647, 1) == 8 && fuse_cap(2147483647, 2147483647) == 2);   // the clamp
    CHECK(fuse_cap(4, 1) == 4 && fuse_cap(8, 1) == 8 && fuse_cap(4, 2) == 2 && fuse_cap(8, 2) == 4 && fuse_cap(4, 3) == 2 && fuse_cap(8, 3) == 2);
    CHECK(fuse_cap(4096, 0) == 2 && fuse_cap(4096, -5) == 2 && fuse_cap(0, 512) == 2 && fuse_cap(-4096, 512) == 2 && fuse_cap(0, 0) == 2 && fuse_cap(-1, -1) == 2);
    for (int budget = -2; budget <= 70; ++budget)
        for (int waves = -2; waves <= 70; ++waves) {
            const int c = fuse_cap(budget, waves);
            CHECK(c >= FUSE_DEFAULT && c <= FUSE_MAX);
            if (budget > 0 && waves > 0) CHECK(c == FUSE_DEFAULT || c == FUSE_MAX || (c * waves <= budget && (c + 1) * waves > budget));
            if (budget > 0 && waves > 0 && c == FUSE_MAX) CHECK(FUSE_MAX * waves <= budget);
            if (budget > 0 && waves > 0 && c == FUSE_DEFAULT) CHECK((FUSE_DEFAULT + 1) * waves > budget);
        }

    // ---- the knobs.  UAVQP_CAPTURE_FUSE_WAVES: a positive integer, anything else the default
    CHECK(fuse_waves_from_env(nullptr) == FUSE_WAVES_DEFAULT && fuse_waves_from_env("") == FUSE_WAVES_DEFAULT);
    CHECK(fuse_waves_from_env("0") == FUSE_WAVES_DEFAULT && fuse_waves_from_env("-4") == FUSE_WAVES_DEFAULT && fuse_waves_from_env("x") == FUSE_WAVES_DEFAULT);
    CHECK(fuse_waves_from_env("4x") == FUSE_WAVES_DEFAULT && fuse_waves_from_env("4.5") == FUSE_WAVES_DEFAULT && fuse_waves_from_env(" ") == FUSE_WAVES_DEFAULT);
    CHECK(fuse_waves_from_env("99999999999999999999") == FUSE_WAVES_DEFAULT && fuse_waves_from_env("4294967297") == FUSE_WAVES_DEFAULT);
    CHECK(fuse_waves_from_env("1") == 1 && fuse_waves_from_env("4") == 4 && fuse_waves_from_env("8") == 8 && fuse_waves_from_env("2048") == 2048);
    CHECK(fuse_waves_from_env("4096") == 4096 && fuse_waves_from_env("1000000") == 1000000 && fuse_waves_from_env("2147483647") == 2147483647);
    // UAVQP_CAPTURE_FUSE named or not: 1..8 as fuse_from_env has them, 0 where fuse_from_env falls back to its default
    CHECK(fuse_named_from_env(nullptr) == 0 && fuse_named_from_env("") == 0 && fuse_named_from_env("0") == 0 && fuse_named_from_env("9") == 0);
    CHECK(fuse_named_from_env("x") == 0 && fuse_named_from_env("-3") == 0);
    for (int v = 1; v <= FUSE_MAX; ++v) {
        char text[4];
        std::snprintf(text, sizeof text, "%d", v);
        CHECK(fuse_named_from_env(text) == v && fuse_from_env(text) == v);
    }
    CHECK(fuse_from_env(nullptr) == FUSE_DEFAULT && fuse_from_env("9") == FUSE_DEFAULT);   // (unchanged: test_capture_fuse.cpp pins every input)

    // ---- the waves one member adds to a group launch, in the kernel group_kernel_choice picks for a group of its shape
    for (int tile = 4; tile <= 8; tile += 4)
        for (int has8 = 0; has8 <= 1; ++has8)
            for (int n_traj : {8, 12, 16, 20, 24, 4092, 4096, 65536}) {
                const unsigned grid = (unsigned)((n_traj + tile - 1) / tile);
                const bool one = n_traj % tile == 0;
                const int w = member_waves(tile, one, n_traj, grid, has8 != 0);
                for (int members = 2; members <= FUSE_MAX; ++members) {
                    const GroupKernel choice = group_kernel_choice(members, tile, one, n_traj, has8 != 0);
                    if (choice == GROUP_EIGHT_PER_WAVE) CHECK(w == n_traj / 8);
                    if (choice == GROUP_OWN_TILE) CHECK(w == (int)grid);
                }
                if (!one) CHECK(w == (int)grid);   // (never fused: the launch as captured)
            }
    CHECK(member_waves(4, true, 4096, 1024, true) == 512 && member_waves(4, true, 4096, 1024, false) == 1024);
    CHECK(member_waves(4, true, 4092, 1023, true) == 1023 && member_waves(8, true, 4096, 512, true) == 512 && member_waves(8, true, 4096, 512, false) == 512);
    CHECK(member_waves(4, true, 8, 2, true) == 1 && member_waves(4, true, 16, 4, true) == 2 && member_waves(4, true, 12, 3, true) == 3);
    CHECK(member_waves(4, true, 65536, 16384, true) == 8192 && member_waves(4, false, 4094, 1024, true) == 1024);
    // the table of the defaults: headline shape, the batch that is no whole number of eights, a shape without the kernel, a large batch
    CHECK(fuse_cap(4096, waves_of(shape_a())) == 8 && fuse_cap(4096, waves_of(shape_odd())) == 4 && fuse_cap(4096, waves_of(shape_b())) == 4);
    CHECK(fuse_cap(2048, waves_of(shape_a())) == 4 && fuse_cap(2048, waves_of(shape_odd())) == 2 && fuse_cap(2048, waves_of(shape_b())) == 2);
    CHECK(FUSE_WAVES_DEFAULT == 2048);   // (the measurement that chose it: docs/measurement_log.md, 2026-10-21)
    CHECK(fuse_cap(FUSE_WAVES_DEFAULT, waves_of(shape_a())) == 4 && fuse_cap(FUSE_WAVES_DEFAULT, waves_of(shape_odd())) == FUSE_DEFAULT);
    CHECK(fuse_cap(FUSE_WAVES_DEFAULT, member_waves(4, true, 65536, 16384, true)) == FUSE_DEFAULT);
    CHECK(fuse_cap(FUSE_WAVES_DEFAULT, member_waves(4, true, 8, 2, true)) == FUSE_MAX);

    {   // ---- the headline: a rotation of 200 solves over 35 sets on 2 lanes, one status array for all; 512 waves per member.
        // Lane 0 has 103 solves and lane 1 has 97 (tests/cpp/test_capture_fuse.cpp); no group of up to 8 meets its own set again.
        std::vector<Record> rec;
        for (int k = 0; k < 200; ++k) {
            rec.push_back(solve(k % 35));
            rec.back().status = at(STATUS, 4096);
        }
        const std::vector<Shape> shape(200, shape_a());
        const std::vector<char> dead = dead_status_stores(rec);
        const Layout lay = lay_out(rec, dead, 2);
        CHECK(waves_of(shape_a()) == 512);
        const Fused f8 = fuse_groups(rec, dead, lay, shape, caps_for(shape, 4096), 2);
        Ints w0(12, 8), w1(12, 8);
        w0.push_back(7);
        w1.push_back(1);
        CHECK(f8.width == Ints{2} && sizes(f8.group[0][0]) == w0 && sizes(f8.group[0][1]) == w1 && launches(f8) == 26 && f8.fused && f8.side_by_side);
        const Fused f4 = fuse_groups(rec, dead, lay, shape, caps_for(shape, 2048), 2);
        CHECK(launches(f4) == 51 && (f4.group[0][0][0] == Ints{0, 2, 4, 6}));
        const Fused f2 = fuse_groups(rec, dead, lay, shape, caps_for(shape, 1024), 2);
        CHECK(launches(f2) == 52 + 49);   // the plan of the default before the budget: groups of two
        // the same rotation over a batch that is no whole number of eights: 1023 waves per member, 4 members at 4096 and 2 at 2048
        const std::vector<Shape> odd(200, shape_odd());
        CHECK(launches(fuse_groups(rec, dead, lay, odd, caps_for(odd, 4096), 2)) == 51 && launches(fuse_groups(rec, dead, lay, odd, caps_for(odd, 2048), 2)) == 101);
    }
    {   // ---- two shapes with different caps in one capture, one lane.  Budget 4096: shape_a 8 members, shape_b 4.
        std::vector<Record> rec;
        std::vector<Shape> shape;
        for (int k = 0; k < 30; ++k) {
            rec.push_back(solve(k));
            shape.push_back(k < 10 ? shape_a() : k < 20 ? shape_b() : shape_a());
        }
        const std::vector<char> dead = dead_status_stores(rec);
        const Layout lay = lay_out(rec, dead, 1);
        const Ints cap = caps_for(shape, 4096);
        CHECK(cap[0] == 8 && cap[10] == 4 && cap[20] == 8);
        const Fused f = fuse_groups(rec, dead, lay, shape, cap, 1);
        CHECK((sizes(f.group[0][0]) == Ints{8, 2, 4, 4, 2, 8, 2}));
        CHECK(holds(rec, conflicts_of(rec, dead), lay, shape, f, cap, 1, NODES_PER_LANE_MIN));
        // interleaved a b a b ...: every shape change closes the group, whatever the caps
        for (int k = 0; k < 30; ++k) shape[(size_t)k] = k % 2 ? shape_b() : shape_a();
        const Fused g = fuse_groups(rec, dead, lay, shape, caps_for(shape, 4096), 1);
        CHECK(launches(g) == 30 && !g.fused);
        // the cap of a group is that of its FIRST member: caps that differ within one shape (no caller makes them) still give a partition
        Ints odd_caps(30, 2);
        odd_caps[0] = 5;
        const std::vector<Shape> all_a(30, shape_a());
        const Fused h = fuse_groups(rec, dead, lay, all_a, odd_caps, 1);
        CHECK(sizes(h.group[0][0])[0] == 5 && sizes(h.group[0][0])[1] == 2 && launches(h) == 1 + 12 + 1);
        // caps above what the kernarg struct holds are cut to it, caps below one give every node its own launch, a vector of the wrong size nothing
        CHECK((sizes(fuse_groups(rec, dead, lay, all_a, Ints(30, 99), 1).group[0][0]) == Ints{8, 8, 8, 6}));
        CHECK(launches(fuse_groups(rec, dead, lay, all_a, Ints(30, 0), 1)) == 30 && launches(fuse_groups(rec, dead, lay, all_a, Ints(30, -7), 1)) == 30);
        CHECK(fuse_groups(rec, dead, lay, all_a, Ints(29, 4), 1).group.empty() && fuse_groups(rec, dead, lay, all_a, Ints(), 1).group.empty());
    }

    // ---- 500 random captures: the per-node overload with a uniform vector is the int-F form, and with the caps of a budget it holds
    // the brute-force statement
    int n_fused = 0, n_two_caps = 0, n_closed_by_cap = 0;
    for (int t = 0; t < 500; ++t) {
        std::vector<Record> rec;
        std::vector<Shape> shape;
        random_capture(rec, shape);
        const std::vector<char> dead = dead_status_stores(rec);
        const std::vector<char> cf = conflicts_of(rec, dead);
        bool any_fused = false, two_caps = false, closed_by_cap = false;
        for (int lanes = 1; lanes <= LANES_MAX; ++lanes) {
            const Layout lay = lay_out(rec, dead, lanes);
            for (int per_lane = 1; per_lane <= 16; per_lane += 15) {
                const int Fs[7] = {-1, 1, 2, 3, 4, 8, 99};
                for (int F : Fs) {
                    const Fused a = fuse_groups(rec, dead, lay, shape, F, lanes, per_lane);
                    const Fused b = fuse_groups(rec, dead, lay, shape, Ints(rec.size(), F), lanes, per_lane);
                    CHECK(a.group == b.group && a.width == b.width && a.fused == b.fused && a.side_by_side == b.side_by_side);
                }
                const int budgets[4] = {512, 1024, 2048, 4096};
                for (int budget : budgets) {
                    const Ints cap = caps_for(shape, budget);
                    const Fused f = fuse_groups(rec, dead, lay, shape, cap, lanes, per_lane);
                    CHECK(holds(rec, cf, lay, shape, f, cap, lanes, per_lane));
                    if (lanes == 2 && budget == 4096) any_fused = any_fused || f.fused;
                    if (lanes > 2) continue;
                    bool big = false, small = false;
                    for (const auto& stage : f.group)
                        for (const Chain& chain : stage)
                            for (size_t g = 0; g < chain.size(); ++g) {
                                big = big || chain[g].size() > 4;
                                small = small || (chain[g].size() == 4 && cap[(size_t)chain[g][0]] == 4);
                                if (g + 1 < chain.size() && (int)chain[g].size() == cap[(size_t)chain[g][0]] && chain[g].size() < (size_t)FUSE_MAX) closed_by_cap = true;
                            }
                    two_caps = two_caps || (big && small);
                }
            }
        }
        n_fused += any_fused;
        n_two_caps += two_caps;
        n_closed_by_cap += closed_by_cap;
    }
    std::printf("random captures: %d of 500 with a group of two or more on 2 lanes at a budget of 4096; on 1 or 2 lanes at any of the budgets, %d with a group above 4 next to one full at a cap of 4, %d with a group closed by a cap below 8\n",
                n_fused, n_two_caps, n_closed_by_cap);
    CHECK(2 * n_fused >= 500);    // otherwise the property holds vacuously
    CHECK(n_two_caps >= 10 && n_closed_by_cap >= 50);

    if (failures == 0) std::printf("capture_fuse_waves OK\n");
    return failures == 0 ? 0 : 1;
}
