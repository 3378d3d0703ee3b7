// Host-only test of the dependency analysis behind uavqp_capture_end (uav_motion_planning_amd/csrc/uavqp_capture.h): a missing edge is
// two solves racing on one buffer when a graph is replayed, so the rules are pinned here, without the HIP runtime.  Compiled and run by
// tests/test_capture_deps.py.
#include <cstdint>
#include <cstdio>
#include <utility>
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
static const uintptr_t STATUS = 0x900000;
typedef std::vector<int> Edges;
static bool none_dead(const Plan& p) {
    for (char d : p.status_dead)
        if (d) return false;
    return true;
}
// is `from` an ancestor of `to` along the plan's edges?
static bool reaches(const Plan& p, int from, int to) {
    if (from == to) return true;
    for (int i : p.preds[to])
        if (i >= from && reaches(p, from, i)) return true;
    return false;
}

int main() {
    // ranges: half-open, touching is no overlap, nothing overlaps the empty range
    CHECK(!at(100, 50).overlaps(at(150, 10)) && !at(150, 10).overlaps(at(100, 50)));
    CHECK(at(100, 51).overlaps(at(150, 10)) && at(150, 10).overlaps(at(100, 51)));
    CHECK(!Range().overlaps(at(0, 100)) && !at(0, 100).overlaps(Range()) && !at(0, 100).covers(Range()));
    CHECK(at(100, 50).covers(at(100, 50)) && at(100, 50).covers(at(110, 40)) && !at(100, 50).covers(at(110, 41)));
    CHECK(range_of(nullptr, 64).empty() && range_of((const void*)0x40, 0).empty() && range_of((const void*)0x40, 8).hi == 0x48);

    {   // disjoint records: lane edges only; at most `lanes` chains
        std::vector<Record> rec;
        for (int k = 0; k < 10; ++k) rec.push_back(solve(k));
        for (int lanes = 2; lanes <= 8; ++lanes) {
            const Plan p = analyse(rec, lanes);
            CHECK(p.parallel && none_dead(p));
            for (int k = 0; k < 10; ++k) CHECK(p.preds[k] == (k >= lanes ? Edges{k - lanes} : Edges{}));
        }
        const Plan chain = analyse(rec, 1);   // one lane: the chain as captured
        CHECK(!chain.parallel && none_dead(chain));
        for (int k = 0; k < 10; ++k) CHECK(chain.preds[k] == (k >= 1 ? Edges{k - 1} : Edges{}));
        CHECK(!analyse(std::vector<Record>(), 4).parallel && !analyse(std::vector<Record>(1, solve(0)), 4).parallel);
    }
    {   // read-after-write: solve 2 reads its durations out of solve 0's coefficients
        std::vector<Record> rec = {solve(0), solve(1), solve(2), solve(3)};
        rec[2].read[1] = at(rec[0].coeff.lo + 0x10, 0x100);
        const Plan p = analyse(rec, 4);
        CHECK(p.preds[0].empty() && p.preds[1].empty() && p.preds[3].empty() && p.preds[2] == Edges{0} && p.parallel);
    }
    {   // write-after-read: solve 1 writes its coefficients over solve 0's boundary values
        std::vector<Record> rec = {solve(0), solve(1), solve(2)};
        rec[1].coeff = at(rec[0].read[2].lo + 0x3F8, 0x400);   // the last 8 bytes of them
        const Plan p = analyse(rec, 4);
        CHECK(p.preds[1] == Edges{0} && p.preds[0].empty() && p.preds[2].empty());
    }
    {   // write-after-write: solves 0 and 2 share the coefficient buffer (a rotation over two sets)
        std::vector<Record> rec = {solve(0), solve(1), solve(0), solve(1), solve(0)};
        const Plan p = analyse(rec, 4);
        CHECK(p.preds[2] == Edges{0} && p.preds[3] == Edges{1} && p.preds[4] == Edges{2});   // 0 -> 4 is implied by 0 -> 2 -> 4
        CHECK(p.preds[0].empty() && p.preds[1].empty() && p.parallel);
    }
    {   // only the transitive reduction: 0 -> 1 -> 2 by data, so neither 0 -> 2 by data nor any lane edge below them is listed twice
        std::vector<Record> rec = {solve(0), solve(1), solve(2), solve(3), solve(4)};
        rec[1].read[0] = rec[0].coeff;
        rec[2].read[0] = rec[1].coeff;
        rec[2].read[1] = rec[0].coeff;
        const Plan p = analyse(rec, 2);
        CHECK(p.preds[1] == Edges{0} && p.preds[2] == Edges{1} && p.preds[3] == Edges{1} && (p.preds[4] == Edges{2}));
        CHECK(p.parallel);   // 2 and 3
    }
    {   // ranges that touch end to start do not conflict
        std::vector<Record> rec = {solve(0), solve(1)};
        rec[1].read[0] = at(rec[0].coeff.hi, 0x100);
        rec[1].coeff = at(rec[0].read[0].lo - 0x400, 0x400);
        rec[0].status = at(STATUS, 256);
        rec[1].status = at(STATUS + 256, 256);
        const Plan p = analyse(rec, 4);
        CHECK(p.preds[1].empty() && p.parallel && none_dead(p));
    }
    {   // identical status ranges: every store but the last is dead, and no edge comes of them
        std::vector<Record> rec;
        for (int k = 0; k < 6; ++k) {
            rec.push_back(solve(k));
            rec.back().status = at(STATUS, 256);
        }
        const Plan p = analyse(rec, 4);
        for (int k = 0; k < 6; ++k) {
            CHECK((p.status_dead[k] != 0) == (k < 5));
            CHECK(p.preds[k] == (k >= 4 ? Edges{k - 4} : Edges{}));
        }
        const Plan chain = analyse(rec, 1);   // the chain as captured keeps every store
        CHECK(none_dead(chain));
    }
    {   // a status range that covers a smaller earlier one: the earlier store is dead; the other way round it is a partial overlap
        std::vector<Record> rec = {solve(0), solve(1)};
        rec[0].status = at(STATUS + 64, 64);
        rec[1].status = at(STATUS, 256);
        Plan p = analyse(rec, 4);
        CHECK(p.status_dead[0] && !p.status_dead[1] && p.preds[1].empty() && p.parallel);
        std::swap(rec[0].status, rec[1].status);
        p = analyse(rec, 4);
        CHECK(none_dead(p) && p.preds[1] == Edges{0} && !p.parallel);
    }
    {   // a partial overlap: an edge and no dead store
        std::vector<Record> rec = {solve(0), solve(1), solve(2)};
        rec[0].status = at(STATUS, 256);
        rec[1].status = at(STATUS + 64, 256);
        const Plan p = analyse(rec, 4);
        CHECK(none_dead(p) && p.preds[1] == Edges{0} && p.preds[2].empty());
    }
    {   // a store is kept when something reads the array, or partly overwrites it, before the solve that covers it
        std::vector<Record> rec = {solve(0), solve(1), solve(2)};
        rec[0].status = rec[2].status = at(STATUS, 256);
        rec[1].read[1] = at(STATUS, 64);
        Plan p = analyse(rec, 4);
        CHECK(!p.status_dead[0] && p.preds[1] == Edges{0} && p.preds[2] == Edges{1});   // RAW 0 -> 1, WAR 1 -> 2
        rec[1] = solve(1);
        rec[1].status = at(STATUS + 128, 256);
        p = analyse(rec, 4);
        CHECK(!p.status_dead[0] && !p.status_dead[1] && p.preds[1] == Edges{0} && p.preds[2] == Edges{1});
        rec[1] = solve(1);
        rec[1].status = at(STATUS + 64, 64);    // a smaller one inside: both it and the first are covered by the last
        p = analyse(rec, 4);
        CHECK(!p.status_dead[0] && p.status_dead[1] && p.preds[1].empty() && p.preds[2] == Edges{0});
    }
    {   // a barrier in the middle orders both sides; a dead store does not reach across it
        std::vector<Record> rec;
        for (int k = 0; k < 7; ++k) {
            rec.push_back(solve(k));
            rec.back().status = at(STATUS, 256);
        }
        rec[3] = Record();
        rec[3].barrier = true;
        const Plan p = analyse(rec, 4);
        CHECK(p.preds[0].empty() && p.preds[1].empty() && p.preds[2].empty());
        CHECK((p.preds[3] == Edges{2, 1, 0}));    // (the stores of 0 and 1 are dead: nothing orders them among themselves)
        for (int k = 0; k < 3; ++k) CHECK(reaches(p, k, 3));
        for (int k = 4; k < 7; ++k) CHECK(p.preds[k] == Edges{3});
        CHECK(p.status_dead[0] && p.status_dead[1] && !p.status_dead[2] && !p.status_dead[3]);
        CHECK(p.status_dead[4] && p.status_dead[5] && !p.status_dead[6] && p.parallel);
    }
    {   // a barrier between disjoint solves: all before it, all behind it
        std::vector<Record> rec = {solve(0), solve(1), Record(), solve(2), solve(3)};
        rec[2].barrier = true;
        const Plan p = analyse(rec, 4);
        CHECK(p.preds[0].empty() && p.preds[1].empty() && (p.preds[2] == Edges{1, 0}) && p.preds[3] == Edges{2} && p.preds[4] == Edges{2});
        CHECK(p.parallel);
        std::vector<Record> only = {solve(0), Record(), solve(1)};
        only[1].barrier = true;
        CHECK(!analyse(only, 4).parallel);
    }
    // more records than the analysis takes: the chain
    {
        std::vector<Record> rec;
        for (size_t k = 0; k < NODES_MAX + 1; ++k) rec.push_back(solve((int)(k % 64)));
        const Plan p = analyse(rec, 4);
        CHECK(!p.parallel && p.preds[NODES_MAX] == Edges{(int)NODES_MAX - 1});
    }

    {   // stages of a replay: the lanes (node k: lane k % lanes) meet only in front of a node that waits for another lane
        std::vector<Record> rec;
        for (int k = 0; k < 12; ++k) rec.push_back(solve(k));
        CHECK(stage_starts(analyse(rec, 4), 4) == Edges{0});             // disjoint: one stage
        CHECK(stage_starts(analyse(rec, 1), 1) == Edges{0});
        rec.clear();
        for (int k = 0; k < 12; ++k) rec.push_back(solve(k % 4));        // a rotation over as many sets as lanes: every conflict inside a lane
        CHECK(stage_starts(analyse(rec, 4), 4) == Edges{0});
        rec.clear();
        for (int k = 0; k < 12; ++k) rec.push_back(solve(k % 5));        // over five sets: node 5 waits for node 0 of another lane, node 10 for 5
        CHECK((stage_starts(analyse(rec, 4), 4) == Edges{0, 5, 10}));
        rec.clear();
        for (int k = 0; k < 7; ++k) rec.push_back(solve(k));
        rec[3] = Record();
        rec[3].barrier = true;                                           // a barrier is a stage of its own
        CHECK((stage_starts(analyse(rec, 4), 4) == Edges{0, 3, 4}));
        CHECK(stage_starts(analyse(std::vector<Record>(), 4), 4).empty());
    }

    // a lane is used where the stage has 16 launches for it: short stages replay as the chain they were captured as
    CHECK(lanes_that_pay(1, 4) == 1 && lanes_that_pay(20, 4) == 1 && lanes_that_pay(31, 4) == 1 && lanes_that_pay(32, 4) == 2);
    CHECK(lanes_that_pay(35, 4) == 2 && lanes_that_pay(63, 4) == 3 && lanes_that_pay(64, 4) == 4 && lanes_that_pay(1000, 4) == 4);
    CHECK(lanes_that_pay(1000, 8) == 8 && lanes_that_pay(1000, 2) == 2 && lanes_that_pay(1000, 1) == 1 && lanes_that_pay(0, 4) == 1);

    CHECK(lanes_that_pay(12, 4, 1) == 4 && lanes_that_pay(2, 4, 1) == 2 && lanes_that_pay(1, 4, 1) == 1 && lanes_that_pay(12, 4, 4) == 3);
    CHECK(lane_nodes_from_env(nullptr) == 16 && lane_nodes_from_env("") == 16 && lane_nodes_from_env("1") == 1 && lane_nodes_from_env("64") == 64);
    CHECK(lane_nodes_from_env("0") == 16 && lane_nodes_from_env("-3") == 16 && lane_nodes_from_env("x") == 16);

    // the lane count: UAVQP_CAPTURE_LANES 1..8, default 4; fewer than 4 hardware queues: the chain
    CHECK(lanes_from_env(nullptr, nullptr) == 4 && lanes_from_env("", "") == 4);
    CHECK(lanes_from_env("1", nullptr) == 1 && lanes_from_env("2", nullptr) == 2 && lanes_from_env("8", nullptr) == 8);
    CHECK(lanes_from_env("0", nullptr) == 4 && lanes_from_env("9", nullptr) == 4 && lanes_from_env("x", nullptr) == 4);
    CHECK(lanes_from_env(nullptr, "4") == 4 && lanes_from_env(nullptr, "32") == 4 && lanes_from_env("8", "4") == 8);
    CHECK(lanes_from_env(nullptr, "3") == 1 && lanes_from_env("8", "2") == 1 && lanes_from_env(nullptr, "1") == 1);

    if (failures == 0) std::printf("capture_deps OK\n");
    return failures == 0 ? 0 : 1;
}
