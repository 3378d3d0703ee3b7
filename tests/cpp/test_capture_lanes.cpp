// Host-only test of the lane layout behind uavqp_capture_end (uav_motion_planning_amd/csrc/uavqp_capture.h: lay_out): two conflicting
// solves that end up in different lanes of one stage race on a buffer when the graph is replayed, so the layout is pinned here, without
// the HIP runtime: a handful of captures by hand, then 500 random ones against the brute-force rule.  Compiled and run by
// tests/test_capture_lanes.py, once plain and once under the address and undefined-behaviour sanitizers.
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

static Layout lay(const std::vector<Record>& rec, int lanes) { return lay_out(rec, dead_status_stores(rec), lanes); }
static Ints loads(const Layout& l, int lanes) {
    Ints c((size_t)lanes, 0);
    for (int x : l.lane) ++c[(size_t)x];
    return c;
}
static Ints stage_of(const Layout& l) {
    Ints st(l.lane.size(), -1);
    for (size_t s = 0; s < l.starts.size(); ++s)
        for (size_t k = (size_t)l.starts[s]; k < (s + 1 < l.starts.size() ? (size_t)l.starts[s + 1] : l.lane.size()); ++k) st[k] = (int)s;
    return st;
}
// does some stage keep two lanes busy?  Counted as the distinct lanes of every stage, whichever lane a stage starts in: independent of
// how the function under test sets its flag
static bool two_busy(const Layout& l) {
    const Ints st = stage_of(l);
    for (size_t s = 0; s < l.starts.size(); ++s) {
        unsigned seen = 0;
        for (size_t k = 0; k < l.lane.size(); ++k)
            if (st[k] == (int)s) seen |= 1u << l.lane[k];
        if (seen & (seen - 1)) return true;
    }
    return false;
}

// ---- the random captures of the property test: a fixed-seed generator, nothing of the function under test in it
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % below;
}
static std::vector<Record> random_capture() {
    const int sets = 1 + (int)rnd(7), n = 2 + (int)rnd(59);
    const int status_mode = (int)rnd(4);         // 0 none, 1 one shared array, 2 one array per set, 3 views shifted into each other
    const bool rotate = rnd(3) != 0;             // a rotation over the sets, or sets at random
    const bool with_barriers = rnd(4) == 0, with_aliases = rnd(2) == 0;
    std::vector<Record> rec;
    for (int k = 0; k < n; ++k) {
        if (with_barriers && rnd(12) == 0) {
            rec.push_back(barrier());
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
        if (with_aliases && rnd(20) == 0) x.read[1] = at(STATUS + 32, 64);   // durations read out of the status array
        rec.push_back(x);
    }
    return rec;
}
// the brute-force rule: every conflicting pair is in different stages or in one lane, also after the lanes are folded onto w
static bool ordered(const std::vector<Record>& rec, const std::vector<char>& dead, const Layout& l, int lanes) {
    const Ints st = stage_of(l);
    for (size_t k = 0; k < rec.size(); ++k)
        for (size_t i = 0; i < k; ++i) {
            if (!conflict(rec[i], dead[i] != 0, rec[k], dead[k] != 0)) continue;
            if (st[i] > st[k]) return false;
            if (st[i] < st[k]) continue;
            for (int w = 1; w <= lanes; ++w)
                if (l.lane[i] % w != l.lane[k] % w) return false;
        }
    return true;
}

int main() {
    {   // a rotation over five sets on four lanes: ONE stage, node k + 5 in the lane of node k (lane k % 4 cuts it at 0, 5, 10)
        std::vector<Record> rec;
        for (int k = 0; k < 12; ++k) rec.push_back(solve(k % 5));
        const Layout l = lay(rec, 4);
        CHECK(l.starts == Ints{0} && l.parallel);
        CHECK((l.lane == Ints{0, 1, 2, 3, 0, 0, 1, 2, 3, 0, 0, 1}));
        CHECK((stage_starts(analyse(rec, 4), 4) == Ints{0, 5, 10}));
        const Layout two = lay(rec, 2);
        CHECK(two.starts == Ints{0} && (two.lane == Ints{0, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1}));
    }
    {   // the headline: 200 solves over 35 sets.  Sets 0..34 go to lanes 0 1 2 3 0 1 ... (9 / 9 / 9 / 8 sets); sets 0..24 are solved six
        // times and sets 25..34 five times: lane 0 has 7 + 2 of them (52 solves), lanes 1 and 2 have 6 + 3 (51), lane 3 has 6 + 2 (46)
        std::vector<Record> rec;
        for (int k = 0; k < 200; ++k) {
            rec.push_back(solve(k % 35));
            rec.back().status = at(STATUS, 4096);   // one status array for all, as the benchmark has it
        }
        const Layout l = lay(rec, 4);
        CHECK(l.starts == Ints{0} && l.parallel);
        for (int k = 35; k < 200; ++k) CHECK(l.lane[k] == l.lane[k - 35]);
        for (int k = 0; k < 35; ++k) CHECK(l.lane[k] == k % 4);
        CHECK((loads(l, 4) == Ints{52, 51, 51, 46}));
        CHECK(lanes_that_pay(200, 4) == 4);
    }
    {   // a solve that takes its durations from one earlier solve's coefficients and its boundary values from another's: the two are in
        // different lanes, so the lanes meet in front of it
        std::vector<Record> rec = {solve(0), solve(1), solve(2), solve(3), solve(4), solve(5), solve(6)};
        rec[4].read[1] = at(rec[0].coeff.lo + 0x10, 0x100);
        rec[4].read[2] = at(rec[2].coeff.lo, 0x80);
        const Layout l = lay(rec, 4);
        CHECK((l.starts == Ints{0, 4}) && (l.lane == Ints{0, 1, 2, 3, 0, 1, 2}) && l.parallel);
        rec[4].read[2] = solve(4).read[2];    // the durations alone: it follows solve 0 in lane 0, no join
        const Layout one = lay(rec, 4);
        CHECK(one.starts == Ints{0} && (one.lane == Ints{0, 1, 2, 3, 0, 1, 2}));
        rec[4].read[2] = at(rec[3].coeff.lo, 0x80);
        rec[3].coeff = rec[0].coeff;          // both inputs from lane 0 (solve 3 rewrites solve 0's coefficients): still no join
        const Layout same = lay(rec, 4);
        CHECK(same.starts == Ints{0} && (same.lane == Ints{0, 1, 2, 0, 0, 3, 1}));
    }
    {   // a barrier in the middle is alone in its stage, and the stage behind it starts in lane 0 again
        std::vector<Record> rec = {solve(0), solve(1), solve(2), barrier(), solve(3), solve(4), solve(5)};
        const Layout l = lay(rec, 4);
        CHECK((l.starts == Ints{0, 3, 4}) && (l.lane == Ints{0, 1, 2, 0, 0, 1, 2}) && l.parallel);
        std::vector<Record> two = {barrier(), barrier(), solve(0)};
        const Layout b = lay(two, 4);
        CHECK((b.starts == Ints{0, 1, 2}) && (b.lane == Ints{0, 0, 0}) && !b.parallel);
        std::vector<Record> only = {solve(0), barrier(), solve(1)};
        CHECK(!lay(only, 4).parallel);
    }
    {   // a chain of solves on one buffer set: one stage, one lane, nothing side by side
        std::vector<Record> rec(9, solve(3));
        const Layout l = lay(rec, 4);
        CHECK(l.starts == Ints{0} && l.lane == Ints(9, 0) && !l.parallel);
    }
    {   // more nodes than the analysis takes, one lane, no node
        std::vector<Record> rec;
        for (size_t k = 0; k < NODES_MAX + 1; ++k) rec.push_back(solve((int)(k % 64)));
        const Layout l = lay_out(rec, std::vector<char>(rec.size(), 0), 4);
        CHECK(l.starts == Ints{0} && l.lane == Ints(NODES_MAX + 1, 0) && !l.parallel);
        rec.pop_back();
        const Layout full = lay(rec, 4);      // NODES_MAX itself is laid out: 64 sets on 4 lanes
        CHECK(full.starts == Ints{0} && full.parallel && (loads(full, 4) == Ints{1024, 1024, 1024, 1024}));
        rec.resize(10);
        const Layout chain = lay(rec, 1);
        CHECK(chain.starts == Ints{0} && chain.lane == Ints(10, 0) && !chain.parallel);
        const Layout none = lay(std::vector<Record>(), 4);
        CHECK(none.starts.empty() && none.lane.empty() && !none.parallel);
    }
    {   // one status array for all: every store but the last is dead and ties nothing together ...
        std::vector<Record> rec;
        for (int k = 0; k < 8; ++k) {
            rec.push_back(solve(k));
            rec.back().status = at(STATUS, 256);
        }
        const Layout l = lay(rec, 4);
        CHECK(l.starts == Ints{0} && (l.lane == Ints{0, 1, 2, 3, 0, 1, 2, 3}));
        // ... without the dead-store rule every one of them is a write-after-write on the array: a chain
        const Layout live = lay_out(rec, std::vector<char>(rec.size(), 0), 4);
        CHECK(live.starts == Ints{0} && live.lane == Ints(8, 0) && !live.parallel);
        // a live partial overlap: solve 5's view is shifted, so it neither covers solve 4's store nor is covered by solve 6's, and the
        // stores of 4 and 5 stay (6's is dead by 7's).  5 follows 4 into lane 0; 6 is free; 7 overwrites both and follows them
        rec[5].status = at(STATUS + 64, 256);
        const std::vector<char> dead = dead_status_stores(rec);
        CHECK(dead[3] && !dead[4] && !dead[5] && dead[6] && !dead[7]);
        const Layout part = lay_out(rec, dead, 4);
        CHECK(part.starts == Ints{0} && (part.lane == Ints{0, 1, 2, 3, 0, 0, 1, 0}));
    }
    {   // live stores in two lanes that a third solve's view overlaps without covering either: the lanes meet in front of it
        std::vector<Record> rec = {solve(0), solve(1), solve(2), solve(3), solve(4), solve(5)};
        rec[1].status = at(STATUS, 64);
        rec[2].status = at(STATUS + 128, 64);
        rec[4].status = at(STATUS + 32, 128);
        const Layout meet = lay(rec, 4);
        CHECK((meet.starts == Ints{0, 4}) && (meet.lane == Ints{0, 1, 2, 3, 0, 1}));
        rec[4].status = at(STATUS, 192);         // it covers both: their stores are dead, one stage
        const Layout covered = lay(rec, 4);
        CHECK(covered.starts == Ints{0} && (covered.lane == Ints{0, 1, 2, 3, 0, 1}));
    }

    // the lane count of a replay: 2 unless UAVQP_CAPTURE_LANES names one (then lanes_from_env's); fewer than 4 hardware queues: the chain
    CHECK(replay_lanes_from_env(nullptr, nullptr) == 2 && replay_lanes_from_env("", "") == 2 && replay_lanes_from_env(nullptr, "32") == 2);
    CHECK(replay_lanes_from_env("x", nullptr) == 2 && replay_lanes_from_env("0", nullptr) == 2 && replay_lanes_from_env("9", nullptr) == 2);
    CHECK(replay_lanes_from_env("1", nullptr) == 1 && replay_lanes_from_env("2", nullptr) == 2 && replay_lanes_from_env("4", nullptr) == 4);
    CHECK(replay_lanes_from_env("8", "4") == 8 && replay_lanes_from_env("3", "16") == 3);
    CHECK(replay_lanes_from_env(nullptr, "3") == 1 && replay_lanes_from_env("8", "2") == 1 && replay_lanes_from_env("4", "1") == 1);
    CHECK(lanes_from_env(nullptr, nullptr) == LANES_DEFAULT && REPLAY_LANES_DEFAULT == 2);
    CHECK(lanes_that_pay(200, REPLAY_LANES_DEFAULT) == 2 && lanes_that_pay(20, REPLAY_LANES_DEFAULT) == 1);
    {   // the headline on two lanes: one stage, sets 0 2 4 .. 34 in lane 0 (18 sets, 13 of them solved six times) and the odd ones in lane 1
        std::vector<Record> rec;
        for (int k = 0; k < 200; ++k) rec.push_back(solve(k % 35));
        const Layout l = lay(rec, REPLAY_LANES_DEFAULT);
        CHECK(l.starts == Ints{0} && l.parallel && (loads(l, 2) == Ints{103, 97}));
    }

    // 500 random captures against the brute-force rule
    int n_parallel = 0, n_barrier = 0, n_staged = 0;
    for (int t = 0; t < 500; ++t) {
        const std::vector<Record> rec = random_capture();
        const std::vector<char> dead = dead_status_stores(rec);
        bool any_parallel = false;
        for (int lanes = 1; lanes <= LANES_MAX; ++lanes) {
            const Layout l = lay_out(rec, dead, lanes);
            bool shape = l.lane.size() == rec.size() && !l.starts.empty() && l.starts[0] == 0;
            for (size_t s = 1; shape && s < l.starts.size(); ++s) shape = l.starts[s] > l.starts[s - 1] && (size_t)l.starts[s] < rec.size();
            for (size_t k = 0; shape && k < rec.size(); ++k) shape = l.lane[k] >= 0 && l.lane[k] < lanes;
            CHECK(shape);
            if (!shape) continue;
            CHECK(ordered(rec, dead, l, lanes));
            const Ints st = stage_of(l);
            for (size_t k = 0; k < rec.size(); ++k) {
                CHECK(l.lane[(size_t)l.starts[(size_t)st[k]]] == 0);                                     // a stage starts in lane 0
                if (rec[k].barrier && lanes > 1) CHECK(l.starts[(size_t)st[k]] == (int)k && (k + 1 == rec.size() || st[k + 1] != st[k]));   // alone (one lane: one stage)
            }
            CHECK(l.parallel == two_busy(l));
            const Layout again = lay_out(rec, dead, lanes);
            CHECK(again.lane == l.lane && again.starts == l.starts);
            if (lanes == LANES_DEFAULT) {
                any_parallel = l.parallel;
                n_staged += l.starts.size() > 1;
            }
        }
        n_parallel += any_parallel;
        for (const Record& x : rec)
            if (x.barrier) {
                ++n_barrier;
                break;
            }
    }
    std::printf("random captures: %d of 500 with a stage of two or more busy lanes on %d lanes, %d with more than one stage, %d with a barrier\n",
                n_parallel, LANES_DEFAULT, n_staged, n_barrier);
    CHECK(2 * n_parallel >= 500);    // otherwise the property holds vacuously
    CHECK(n_staged >= 50 && n_barrier >= 50);

    if (failures == 0) std::printf("capture_lanes OK\n");
    return failures == 0 ? 0 : 1;
}
