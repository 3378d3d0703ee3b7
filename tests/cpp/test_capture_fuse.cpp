// Host-only test of the grouping behind uavqp_capture_end (uav_motion_planning_amd/csrc/uavqp_capture.h: fuse_groups): the solves of a
// group are replayed as ONE launch, side by side, so two conflicting solves in one group race on a buffer.  The groupings of a handful of
// captures are pinned here, without the HIP runtime, then 500 random captures are checked against the brute-force statement of the rule.
// Compiled and run by tests/test_capture_fuse.py, once plain and once under the address and undefined-behaviour sanitizers.
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

static const int KERNEL_A = 0, KERNEL_B = 0;   // two kernel functions: only their addresses count
// a launch of the one-tile-per-wave instantiation: 1024 waves over 4096 trajectories
static Shape shape_a() {
    Shape s;
    s.fn = &KERNEL_A; s.grid = 1024; s.block = 64; s.n_traj = 4096; s.one = true;
    return s;
}
static Shape shape_b() {   // another kernel function (another (r, M)), same grid
    Shape s = shape_a();
    s.fn = &KERNEL_B;
    return s;
}
static Shape shape_half() {   // the same kernel over half the batch
    Shape s = shape_a();
    s.grid = 512; s.n_traj = 2048;
    return s;
}
static Shape shape_ragged() {   // a launch that does not take the one-tile-per-wave instantiation (n % TILE != 0)
    Shape s = shape_a();
    s.n_traj = 4094; s.one = false;
    return s;
}

static Fused fuse(const std::vector<Record>& rec, const std::vector<Shape>& shape, int lanes, int F, int per_lane = NODES_PER_LANE_MIN) {
    const std::vector<char> dead = dead_status_stores(rec);
    return fuse_groups(rec, dead, lay_out(rec, dead, lanes), shape, F, lanes, per_lane);
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

// ---- the random captures of the property test: a fixed-seed generator, nothing of the function under test in it
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
            const uint32_t pick = rnd(6);
            run = pick == 0 ? shape_b() : pick == 1 ? shape_half() : pick == 2 ? shape_ragged() : shape_a();
        }
        shape.push_back(run);
    }
}

// The brute-force statement of section "Groups" of uavqp_capture.h, from the layout and the records alone.
// `cf` is the conflict relation of the capture, conflict() for every pair, worked out once per capture by the caller.
static bool holds(const std::vector<Record>& rec, const std::vector<char>& cf, const Layout& lay, const std::vector<Shape>& shape, const Fused& f,
                  int F, int lanes, int per_lane) {
    const int n = (int)rec.size();
    auto conflicting = [&](int i, int k) { return cf[(size_t)i * (size_t)n + (size_t)k] != 0; };
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
                if (chain[g].empty() || (int)chain[g].size() > (F < 1 ? 1 : F)) return false;
                fused = fused || chain[g].size() > 1;
                for (int k : chain[g]) {
                    if (k < 0 || k >= n || seen[(size_t)k]++) return false;
                    flat.push_back(k);
                    stage_of[(size_t)k] = (int)s; lane_of[(size_t)k] = l; group_of[(size_t)k] = (int)g;
                }
            }
            for (int k = first; k < last; ++k)
                if (lay.lane[(size_t)k] % f.width[s] == l) want.push_back(k);
            if (flat != want) return false;
            for (size_t g = 0; g < chain.size(); ++g) {
                // members: one shape, the one-tile-per-wave instantiation, no barrier, pairwise conflict-free
                for (size_t x = 0; x < chain[g].size(); ++x)
                    for (size_t y = 0; y < x; ++y) {
                        const int i = chain[g][y], k = chain[g][x];
                        if (rec[(size_t)i].barrier || rec[(size_t)k].barrier || !shape[(size_t)i].one || !shape[(size_t)k].one) return false;
                        if (!same_shape(shape[(size_t)i], shape[(size_t)k])) return false;
                        if (conflicting(i, k)) return false;
                    }
                // a group is closed only for a reason: its successor's first node could not have joined it
                if (g + 1 < chain.size()) {
                    const int k = chain[g + 1][0];
                    bool could = !rec[(size_t)k].barrier && shape[(size_t)k].one && (int)chain[g].size() < F;
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

int main() {
    {   // the headline: a rotation of 200 solves over 35 sets on 2 lanes, one status array for all (every store but the last is dead).
        // Lane 0 has the 18 even sets, lane 1 the 17 odd ones (tests/cpp/test_capture_lanes.cpp): 5 whole rounds and sets 0..24 of a sixth,
        // 5 * 18 + 13 = 103 and 5 * 17 + 12 = 97 solves.  A lane meets a set again after 18 (17) solves, so no group of up to 8 meets its own:
        // the lanes are cut every F solves.   F = 4: 103 = 25 * 4 + 3 and 97 = 24 * 4 + 1, 26 + 25 = 51 launches;
        //                                     F = 8: 103 = 12 * 8 + 7 and 97 = 12 * 8 + 1, 13 + 13 = 26 launches.
        std::vector<Record> rec;
        for (int k = 0; k < 200; ++k) {
            rec.push_back(solve(k % 35));
            rec.back().status = at(STATUS, 4096);
        }
        const std::vector<Shape> shape(200, shape_a());
        const Fused f4 = fuse(rec, shape, 2, 4);
        CHECK(f4.width == Ints{2} && f4.group.size() == 1 && f4.fused && f4.side_by_side);
        Ints want0(25, 4), want1(24, 4);
        want0.push_back(3);
        want1.push_back(1);
        CHECK(sizes(f4.group[0][0]) == want0 && sizes(f4.group[0][1]) == want1 && launches(f4) == 51);
        CHECK((f4.group[0][0][0] == Ints{0, 2, 4, 6}) && (f4.group[0][1][0] == Ints{1, 3, 5, 7}));
        CHECK((f4.group[0][0][4] == Ints{32, 34, 35, 37}));   // sets 32, 34, then round two: sets 0, 2
        CHECK((f4.group[0][0][25] == Ints{195, 197, 199}) && (f4.group[0][1][24] == Ints{198}));
        const Fused f8 = fuse(rec, shape, 2, 8);
        Ints w0(12, 8), w1(12, 8);
        w0.push_back(7);
        w1.push_back(1);
        CHECK(sizes(f8.group[0][0]) == w0 && sizes(f8.group[0][1]) == w1 && launches(f8) == 26);
        // the chain of 20: lanes_that_pay(20, 2) == 1, both lanes of the layout fold onto one and the 20 solves are 20 different sets
        rec.resize(20);
        const Fused chain = fuse(rec, std::vector<Shape>(20, shape_a()), 2, 8);
        CHECK(chain.width == Ints{1} && (sizes(chain.group[0][0]) == Ints{8, 8, 4}) && chain.fused && !chain.side_by_side);
        CHECK((chain.group[0][0][0] == Ints{0, 1, 2, 3, 4, 5, 6, 7}));
    }
    {   // a run that meets its own set again inside a would-be group: the group closes there.  Three sets on one lane, F = 8
        std::vector<Record> rec;
        for (int k = 0; k < 8; ++k) rec.push_back(solve(k % 3));
        const std::vector<Shape> shape(8, shape_a());
        const Fused f = fuse(rec, shape, 1, 8);
        CHECK(f.width == Ints{1} && (f.group[0][0] == Chain{{0, 1, 2}, {3, 4, 5}, {6, 7}}) && f.fused && !f.side_by_side);
        // four sets on two lanes (a lane for every launch): sets 0, 2 and sets 1, 3 alternate in their lanes
        rec.clear();
        for (int k = 0; k < 10; ++k) rec.push_back(solve(k % 4));
        const Fused g = fuse(rec, std::vector<Shape>(10, shape_a()), 2, 4, 1);
        CHECK(g.width == Ints{2} && (g.group[0][0] == Chain{{0, 2}, {4, 6}, {8}}) && (g.group[0][1] == Chain{{1, 3}, {5, 7}, {9}}));
        // the same set twice in a row is never fused
        std::vector<Record> twice = {solve(0), solve(0), solve(1)};
        const Fused t = fuse(twice, std::vector<Shape>(3, shape_a()), 1, 8);
        CHECK((t.group[0][0] == Chain{{0}, {1, 2}}));
    }
    {   // a shape change in mid-run closes the group; a launch that is not one whole tile per wave is alone
        std::vector<Record> rec;
        for (int k = 0; k < 8; ++k) rec.push_back(solve(k));
        std::vector<Shape> shape = {shape_a(), shape_a(), shape_a(), shape_b(), shape_b(), shape_a(), shape_half(), shape_half()};
        const Fused f = fuse(rec, shape, 1, 8);
        CHECK((f.group[0][0] == Chain{{0, 1, 2}, {3, 4}, {5}, {6, 7}}));
        shape[1] = shape_ragged();
        shape[2] = shape_ragged();
        const Fused r = fuse(rec, shape, 1, 8);
        CHECK((r.group[0][0] == Chain{{0}, {1}, {2}, {3, 4}, {5}, {6, 7}}));
    }
    {   // a barrier is alone in its group (one lane: one stage) and in its stage (two lanes)
        std::vector<Record> rec = {solve(0), solve(1), barrier(), solve(2), solve(3), solve(4)};
        std::vector<Shape> shape(6, shape_a());
        shape[2] = Shape();
        const Fused one = fuse(rec, shape, 1, 8);
        CHECK(one.width == Ints{1} && (one.group[0][0] == Chain{{0, 1}, {2}, {3, 4, 5}}));
        const Fused two = fuse(rec, shape, 2, 8, 1);
        CHECK((two.width == Ints{2, 1, 2}));
        CHECK(two.group[0][0] == Chain{Ints{0}} && two.group[0][1] == Chain{Ints{1}} && two.group[1][0] == Chain{Ints{2}});
        CHECK((two.group[2][0] == Chain{Ints{3, 5}}) && two.group[2][1] == Chain{Ints{4}});
        CHECK(two.fused && two.side_by_side);
    }
    {   // F = 1 (and anything below): every solve its own launch -- the chains of lay_out, folded onto the lanes that pay
        std::vector<Record> rec;
        for (int k = 0; k < 70; ++k) rec.push_back(solve(k % 5));
        const std::vector<Shape> shape(70, shape_a());
        const std::vector<char> dead = dead_status_stores(rec);
        for (int lanes = 1; lanes <= 4; ++lanes) {
            const Layout lay = lay_out(rec, dead, lanes);
            for (int F = -1; F <= 1; ++F) {
                const Fused f = fuse_groups(rec, dead, lay, shape, F, lanes);
                CHECK(!f.fused && f.side_by_side == (lanes > 1) && launches(f) == 70 && f.width == Ints{lanes_that_pay(70, lanes)});
                for (int l = 0; l < f.width[0]; ++l) {
                    Ints flat, want;
                    for (const Ints& g : f.group[0][(size_t)l]) flat.insert(flat.end(), g.begin(), g.end());
                    for (int k = 0; k < 70; ++k)
                        if (lay.lane[(size_t)k] % f.width[0] == l) want.push_back(k);
                    CHECK(flat == want);
                }
            }
        }
        // more than the kernarg struct holds is cut to it; arguments that do not fit the records give nothing
        const Fused big = fuse_groups(rec, dead, lay_out(rec, dead, 1), shape, 99, 1);
        CHECK((sizes(big.group[0][0]) == Ints(14, 5)));     // (five sets: a group meets its own after five)
        std::vector<Record> many;
        for (int k = 0; k < 40; ++k) many.push_back(solve(k));
        const std::vector<char> none(40, 0);
        CHECK((sizes(fuse_groups(many, none, lay_out(many, none, 1), std::vector<Shape>(40, shape_a()), 99, 1).group[0][0]) == Ints(5, FUSE_MAX)));
        CHECK(fuse_groups(many, none, lay_out(many, none, 1), std::vector<Shape>(39, shape_a()), 4, 1).group.empty());
        CHECK(fuse_groups(std::vector<Record>(), std::vector<char>(), Layout(), std::vector<Shape>(), 4, 2).group.empty());
    }
    {   // status stores: solve 1's view is shifted against solve 0's and covered by solve 2's, so its store is dead (never made) and it
        // goes along with solve 0; solve 2's store is live and overlaps solve 0's: write-after-write, the group closes
        std::vector<Record> rec = {solve(0), solve(1), solve(2)};
        rec[0].status = at(STATUS, 256);
        rec[1].status = at(STATUS + 64, 256);
        rec[2].status = at(STATUS + 64, 256);
        const std::vector<char> dead = dead_status_stores(rec);
        CHECK(!dead[0] && dead[1] && !dead[2]);
        const Fused f = fuse(rec, std::vector<Shape>(3, shape_a()), 1, 8);
        CHECK((f.group[0][0] == Chain{{0, 1}, {2}}));
        // without the dead-store flags every pair is a write-after-write
        const std::vector<char> none(3, 0);
        CHECK((fuse_groups(rec, none, lay_out(rec, none, 1), std::vector<Shape>(3, shape_a()), 8, 1).group[0][0] == Chain{{0}, {1}, {2}}));
    }

    // the knob: 1..8, anything else the default
    CHECK(fuse_from_env(nullptr) == FUSE_DEFAULT && fuse_from_env("") == FUSE_DEFAULT && fuse_from_env("0") == FUSE_DEFAULT);
    CHECK(fuse_from_env("9") == FUSE_DEFAULT && fuse_from_env("x") == FUSE_DEFAULT && fuse_from_env("-3") == FUSE_DEFAULT);
    CHECK(fuse_from_env("1") == 1 && fuse_from_env("2") == 2 && fuse_from_env("4") == 4 && fuse_from_env("8") == 8);
    CHECK(FUSE_DEFAULT >= 1 && FUSE_DEFAULT <= FUSE_MAX && FUSE_MAX == 8);

    // 500 random captures against the brute-force statement
    int n_fused = 0, n_barrier = 0, n_cut_by_conflict = 0;
    for (int t = 0; t < 500; ++t) {
        std::vector<Record> rec;
        std::vector<Shape> shape;
        random_capture(rec, shape);
        const std::vector<char> dead = dead_status_stores(rec);
        bool any_fused = false, any_cut = false;
        const size_t n = rec.size();
        std::vector<char> cf(n * n, 0);
        for (size_t k = 0; k < n; ++k)
            for (size_t i = 0; i < k; ++i) cf[i * n + k] = conflict(rec[i], dead[i] != 0, rec[k], dead[k] != 0);
        for (int lanes = 1; lanes <= LANES_MAX; ++lanes) {
            const Layout lay = lay_out(rec, dead, lanes);
            const int Fs[5] = {1, 2, 3, 4, 8};
            for (int F : Fs)
                for (int per_lane = 1; per_lane <= 16; per_lane += 15) {
                    const Fused f = fuse_groups(rec, dead, lay, shape, F, lanes, per_lane);
                    CHECK(holds(rec, cf, lay, shape, f, F, lanes, per_lane));
                    const Fused again = fuse_groups(rec, dead, lay, shape, F, lanes, per_lane);
                    CHECK(again.group == f.group && again.width == f.width);
                    if (F == 1) CHECK(!f.fused && launches(f) == (int)rec.size());
                    if (lanes == 2 && F == 4) {
                        any_fused = any_fused || f.fused;
                        for (const auto& stage : f.group)
                            for (const Chain& chain : stage)
                                for (size_t g = 0; g + 1 < chain.size(); ++g)
                                    if (chain[g].size() < 4 && !rec[(size_t)chain[g + 1][0]].barrier && !rec[(size_t)chain[g][0]].barrier &&
                                        same_shape(shape[(size_t)chain[g][0]], shape[(size_t)chain[g + 1][0]]) && shape[(size_t)chain[g][0]].one)
                                        any_cut = true;
                }
            }
        }
        n_fused += any_fused;
        n_cut_by_conflict += any_cut;
        for (const Record& x : rec)
            if (x.barrier) {
                ++n_barrier;
                break;
            }
    }
    std::printf("random captures: %d of 500 with a group of two or more on 2 lanes at F = 4, %d with a group closed by a conflict, %d with a barrier\n",
                n_fused, n_cut_by_conflict, n_barrier);
    CHECK(2 * n_fused >= 500);    // otherwise the property holds vacuously
    CHECK(n_cut_by_conflict >= 50 && n_barrier >= 50);

    if (failures == 0) std::printf("capture_fuse OK\n");
    return failures == 0 ? 0 : 1;
}
