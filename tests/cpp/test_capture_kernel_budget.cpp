// Host-only test of the budget of waves PER KERNEL (uav_motion_planning_amd/csrc/uavqp_capture.h: fuse_waves_named_from_env,
// fuse_budget, group_cap, FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT): where UAVQP_CAPTURE_FUSE_WAVES names no budget, a group that runs the
// eight-per-wave kernel is cut by that kernel's own default and every other group by FUSE_WAVES_DEFAULT; a named budget holds for every
// kernel and a named count (UAVQP_CAPTURE_FUSE) overrides both, as before.  Without the HIP runtime: the new parser at its edges and
// against fuse_waves_from_env, the cap of a group under the three settings for the four kinds of shape, the benchmark's rotation and
// the batch that is no whole number of eights under the defaults, every small member at FUSE_MAX under either default, and 500 random
// captures on which a named budget or count gives exactly the plan of the rule before (fuse_cap over member_waves; the int-F form).
// Compiled and run by tests/test_capture_kernel_budget.py, once plain and once under the address and undefined-behaviour sanitizers.
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

// What a test knows of a launch beyond its Shape: the tile of the captured kernel and whether its (r, M) has an eight-per-wave kernel.
struct Kind {
    Shape shape;
    int tile;
    bool has8;
};
static const int KERNEL_A = 0, KERNEL_B = 0, KERNEL_C = 0;   // only their addresses count
static Kind kind(const void* fn, int tile, int n_traj, bool one, bool has8) {
    Kind k;
    k.shape.fn = fn; k.shape.grid = (unsigned)((n_traj + tile - 1) / tile); k.shape.block = 64; k.shape.n_traj = n_traj; k.shape.one = one;
    k.tile = tile; k.has8 = has8;
    return k;
}
static Kind kind_a() { return kind(&KERNEL_A, 4, 4096, true, true); }        // the headline: 1024 waves as captured, 512 in the eight-per-wave kernel
static Kind kind_b() { return kind(&KERNEL_B, 4, 4096, true, false); }       // a shape without an eight-per-wave kernel: 1024 waves per member
static Kind kind_odd() { return kind(&KERNEL_A, 4, 4092, true, true); }      // n % 8 != 0: the 16-lane group kernel, 1023 waves per member
static Kind kind_tile8() { return kind(&KERNEL_C, 8, 4096, true, false); }   // a launch of the 8-lane shape: 512 waves per member, its own group kernel
static Kind kind_half() { return kind(&KERNEL_A, 4, 2048, true, true); }     // 256 waves per member
static Kind kind_ragged() { return kind(&KERNEL_A, 4, 4094, false, true); }  // not the one-tile-per-wave instantiation: never fused
static int cap_of(const Kind& k, int fuse_named, int waves_named) {
    return group_cap(fuse_named, waves_named, k.tile, k.shape.one, k.shape.n_traj, k.shape.grid, k.has8);
}
static int old_cap_of(const Kind& k, int budget) {   // the rule before: one budget for every kernel
    return fuse_cap(budget, member_waves(k.tile, k.shape.one, k.shape.n_traj, k.shape.grid, k.has8));
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

// ---- random captures: the fixed-seed generator of test_capture_fuse_waves.cpp, restated with the kinds above
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % below;
}
static void random_capture(std::vector<Record>& rec, std::vector<Kind>& kinds) {
    const int sets = 1 + (int)rnd(9), n = 2 + (int)rnd(59);
    const int status_mode = (int)rnd(4);         // 0 none, 1 one shared array, 2 one array per set, 3 views shifted into each other
    const bool rotate = rnd(3) != 0;             // a rotation over the sets, or sets at random
    const bool with_barriers = rnd(4) == 0, with_aliases = rnd(2) == 0;
    const int shape_mode = (int)rnd(3);          // 0 one shape, 1 runs of two shapes, 2 shapes at random
    rec.clear();
    kinds.clear();
    Kind run = kind_a();
    for (int k = 0; k < n; ++k) {
        if (with_barriers && rnd(12) == 0) {
            rec.push_back(barrier());
            kinds.push_back(kind(nullptr, 4, 0, false, false));
            kinds.back().shape = Shape();
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
        rec.push_back(x);
        if (shape_mode == 1 && rnd(7) == 0) run = run.shape.fn == &KERNEL_A ? kind_b() : kind_a();
        if (shape_mode == 2) {
            const uint32_t pick = rnd(8);
            run = pick == 0 ? kind_b() : pick == 1 ? kind_half() : pick == 2 ? kind_ragged() : pick == 3 ? kind_odd() : pick == 4 ? kind_tile8() : kind_a();
        }
        kinds.push_back(run);
    }
}
static bool same_plan(const Fused& a, const Fused& b) { return a.group == b.group && a.width == b.width && a.fused == b.fused && a.side_by_side == b.side_by_side; }

int main() {
    // ---- the constants: the other kernels keep 2048; the eight-per-wave kernel's default is one of the measured candidates
    CHECK(FUSE_WAVES_DEFAULT == 2048 && FUSE_DEFAULT == 2 && FUSE_MAX == 8);
    CHECK(FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT == 2048 || FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT == 3072 || FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT == 4096);
    CHECK(FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT == 2048);   // (the measurements that kept it there: docs/measurement_log.md, 2026-10-21, second entry)

    // ---- the parser that says "names none": a positive integer that fits an int, anything else 0
    CHECK(fuse_waves_named_from_env(nullptr) == 0 && fuse_waves_named_from_env("") == 0);
    CHECK(fuse_waves_named_from_env("0") == 0 && fuse_waves_named_from_env("00") == 0 && fuse_waves_named_from_env("-0") == 0);
    CHECK(fuse_waves_named_from_env("-1") == 0 && fuse_waves_named_from_env("-4096") == 0 && fuse_waves_named_from_env("-99999999999999999999") == 0);
    CHECK(fuse_waves_named_from_env("4x") == 0 && fuse_waves_named_from_env("4096 ") == 0 && fuse_waves_named_from_env("4.5") == 0 && fuse_waves_named_from_env("4096\n") == 0);
    CHECK(fuse_waves_named_from_env(" 4096") == 0 && fuse_waves_named_from_env("+4096") == 0 && fuse_waves_named_from_env("x") == 0 && fuse_waves_named_from_env(" ") == 0);
    CHECK(fuse_waves_named_from_env("0x1000") == 0 && fuse_waves_named_from_env("1e3") == 0);
    CHECK(fuse_waves_named_from_env("2147483648") == 0 && fuse_waves_named_from_env("4294967297") == 0 && fuse_waves_named_from_env("9223372036854775807") == 0);
    CHECK(fuse_waves_named_from_env("9223372036854775808") == 0 && fuse_waves_named_from_env("99999999999999999999") == 0);
    CHECK(fuse_waves_named_from_env("1") == 1 && fuse_waves_named_from_env("8") == 8 && fuse_waves_named_from_env("2048") == 2048 && fuse_waves_named_from_env("3072") == 3072);
    CHECK(fuse_waves_named_from_env("4096") == 4096 && fuse_waves_named_from_env("0004096") == 4096 && fuse_waves_named_from_env("2147483647") == 2147483647);
    {   // fuse_waves_from_env is the same parse with FUSE_WAVES_DEFAULT for "none" (its own inputs: test_capture_fuse_waves.cpp)
        const char* texts[] = {nullptr, "", "0", "-4", "x", "4x", "4.5", " ", "99999999999999999999", "4294967297", "1", "4", "2048", "4096", "1000000", "2147483647", "2147483648", "+7", " 7"};
        for (const char* t : texts) {
            const int named = fuse_waves_named_from_env(t);
            CHECK(named >= 0 && fuse_waves_from_env(t) == (named ? named : FUSE_WAVES_DEFAULT));
        }
    }

    // ---- the budget and the cap of a group, for the four kinds of shape
    const Kind a = kind_a(), b = kind_b(), odd = kind_odd(), t8 = kind_tile8();
    CHECK(group_kernel_choice(2, a.tile, true, a.shape.n_traj, a.has8) == GROUP_EIGHT_PER_WAVE && group_kernel_choice(2, b.tile, true, b.shape.n_traj, b.has8) == GROUP_OWN_TILE);
    CHECK(group_kernel_choice(2, odd.tile, true, odd.shape.n_traj, odd.has8) == GROUP_OWN_TILE && group_kernel_choice(2, t8.tile, true, t8.shape.n_traj, t8.has8) == GROUP_OWN_TILE);
    // not set: the eight-per-wave kernel has its own default, everything else FUSE_WAVES_DEFAULT (also tile 8 with the flag set: the kernel is tile 4's)
    CHECK(fuse_budget(0, 4, true, 4096, true) == FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT && fuse_budget(0, 4, true, 4096, false) == FUSE_WAVES_DEFAULT);
    CHECK(fuse_budget(0, 4, true, 4092, true) == FUSE_WAVES_DEFAULT && fuse_budget(0, 8, true, 4096, false) == FUSE_WAVES_DEFAULT && fuse_budget(0, 8, true, 4096, true) == FUSE_WAVES_DEFAULT);
    CHECK(fuse_budget(0, 4, false, 4096, true) == FUSE_WAVES_DEFAULT && fuse_budget(-3, 4, true, 4096, true) == FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT);
    CHECK(cap_of(a, 0, 0) == fuse_cap(FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT, 512) && cap_of(a, 0, 0) == 4);
    CHECK(cap_of(b, 0, 0) == 2 && cap_of(odd, 0, 0) == 2 && cap_of(t8, 0, 0) == 4 && cap_of(kind_ragged(), 0, 0) == 2);
    CHECK(cap_of(kind_half(), 0, 0) == 8 && cap_of(kind(&KERNEL_A, 4, 65536, true, true), 0, 0) == 2);
    // a named budget: every kernel alike, the rule before
    for (int budget : {1, 512, 1023, 1024, 2048, 3072, 4096, 8192, 2147483647}) {
        CHECK(fuse_budget(budget, 4, true, 4096, true) == budget && fuse_budget(budget, 4, true, 4092, true) == budget && fuse_budget(budget, 8, true, 4096, false) == budget);
        for (const Kind& k : {a, b, odd, t8, kind_half(), kind_ragged()}) CHECK(cap_of(k, 0, budget) == old_cap_of(k, budget));
    }
    CHECK(cap_of(a, 0, 4096) == 8 && cap_of(b, 0, 4096) == 4 && cap_of(odd, 0, 4096) == 4 && cap_of(t8, 0, 4096) == 8);
    CHECK(cap_of(a, 0, 2048) == 4 && cap_of(b, 0, 2048) == 2 && cap_of(odd, 0, 2048) == 2 && cap_of(t8, 0, 2048) == 4);
    CHECK(cap_of(a, 0, 3072) == 6 && cap_of(b, 0, 3072) == 3 && cap_of(odd, 0, 3072) == 3 && cap_of(t8, 0, 3072) == 6);
    // a named count: overrides both, for every kind
    for (int F = 1; F <= FUSE_MAX; ++F)
        for (int budget : {0, 1, 2048, 4096})
            for (const Kind& k : {a, b, odd, t8, kind_half(), kind_ragged()}) CHECK(cap_of(k, F, budget) == F);
    CHECK(cap_of(a, 99, 0) == FUSE_MAX);   // (no caller passes one: fuse_named_from_env gives 0..8)

    // ---- small members reach FUSE_MAX under either default: every n with n / 8 <= 256 waves, so the plans of
    // tests/cpp/capture_fuse_waves_plan.cpp (one budget, FUSE_WAVES_DEFAULT where none is named) are those of the library for them
    for (int n = 8; n <= 2048; n += 8) {
        const Kind k = kind(&KERNEL_A, 4, n, true, true);
        CHECK(cap_of(k, 0, 0) == FUSE_MAX && old_cap_of(k, FUSE_WAVES_DEFAULT) == FUSE_MAX);
    }
    CHECK(old_cap_of(kind(&KERNEL_A, 4, 2056, true, true), FUSE_WAVES_DEFAULT) == 7);   // 257 waves: the first size at which the defaults can differ
    for (int n : {12, 20, 36}) {   // no whole number of eights: FUSE_WAVES_DEFAULT either way
        const Kind k = kind(&KERNEL_A, 4, n, true, true);
        CHECK(cap_of(k, 0, 0) == old_cap_of(k, FUSE_WAVES_DEFAULT));
    }

    {   // ---- the headline: a rotation of 200 solves over 35 sets on 2 lanes, one status array for all; 512 waves per member.
        // Lane 0 has 103 solves and lane 1 has 97 (tests/cpp/test_capture_fuse.cpp); no group of up to 8 meets its own set again.
        std::vector<Record> rec;
        for (int k = 0; k < 200; ++k) {
            rec.push_back(solve(k % 35));
            rec.back().status = at(STATUS, 4096);
        }
        const std::vector<char> dead = dead_status_stores(rec);
        const Layout lay = lay_out(rec, dead, 2);
        auto plan = [&](const Kind& k, int fuse_named, int waves_named) {
            return fuse_groups(rec, dead, lay, std::vector<Shape>(200, k.shape), Ints(200, cap_of(k, fuse_named, waves_named)), 2);
        };
        const Fused f = plan(a, 0, 0);   // nothing named: 4 members of 512 waves, 26 + 25 launches
        Ints w0(25, 4), w1(24, 4);
        w0.push_back(3);
        w1.push_back(1);
        CHECK(f.width == Ints{2} && sizes(f.group[0][0]) == w0 && sizes(f.group[0][1]) == w1 && launches(f) == 51 && f.fused && f.side_by_side);
        CHECK((f.group[0][0][0] == Ints{0, 2, 4, 6}));
        {   // a named budget of 4096: 8 members, 13 + 13 launches
            const Fused f8 = plan(a, 0, 4096);
            Ints v0(12, 8), v1(12, 8);
            v0.push_back(7);
            v1.push_back(1);
            CHECK(sizes(f8.group[0][0]) == v0 && sizes(f8.group[0][1]) == v1 && launches(f8) == 26);
        }
        CHECK(launches(plan(a, 0, 2048)) == 51 && launches(plan(a, 0, 3072)) == 18 + 17 && launches(plan(a, 0, 1024)) == 101 && launches(plan(a, 4, 0)) == 51 && launches(plan(a, 1, 0)) == 200);
        // --batch 4092 keeps the plan it had: 2 members of the 16-lane group kernel, 52 + 49 launches
        CHECK(launches(plan(odd, 0, 0)) == 101 && launches(plan(odd, 0, 2048)) == 101 && launches(plan(odd, 0, 4096)) == 51);
        // a shape without an eight-per-wave kernel, and the 8-lane shape
        CHECK(launches(plan(b, 0, 0)) == 101 && launches(plan(t8, 0, 0)) == 51);
    }

    // ---- 500 random captures: with a budget named the plan is that of the rule before; with a count named that of the int-F form;
    // with nothing named only launches that run the eight-per-wave kernel have another cap than before
    int n_fused = 0, n_differ = 0;
    for (int t = 0; t < 500; ++t) {
        std::vector<Record> rec;
        std::vector<Kind> kinds;
        random_capture(rec, kinds);
        std::vector<Shape> shape;
        for (const Kind& k : kinds) shape.push_back(k.shape);
        const std::vector<char> dead = dead_status_stores(rec);
        bool any_fused = false, differ = false;
        for (int lanes = 1; lanes <= 2; ++lanes) {
            const Layout lay = lay_out(rec, dead, lanes);
            for (int budget : {512, 1024, 2048, 3072, 4096}) {
                Ints now, before;
                for (const Kind& k : kinds) {
                    now.push_back(cap_of(k, 0, budget));
                    before.push_back(old_cap_of(k, budget));
                }
                CHECK(now == before);
                const Fused f = fuse_groups(rec, dead, lay, shape, now, lanes, 1);
                CHECK(same_plan(f, fuse_groups(rec, dead, lay, shape, before, lanes, 1)));
                any_fused = any_fused || f.fused;
            }
            for (int F = 1; F <= FUSE_MAX; ++F) {
                Ints now;
                for (const Kind& k : kinds) now.push_back(cap_of(k, F, 4096));
                CHECK(same_plan(fuse_groups(rec, dead, lay, shape, now, lanes, 1), fuse_groups(rec, dead, lay, shape, F, lanes, 1)));
            }
            Ints unset, before;
            for (const Kind& k : kinds) {
                unset.push_back(cap_of(k, 0, 0));
                before.push_back(old_cap_of(k, FUSE_WAVES_DEFAULT));
                const bool eight = group_kernel_choice(2, k.tile, k.shape.one, k.shape.n_traj, k.has8) == GROUP_EIGHT_PER_WAVE;
                if (!eight) CHECK(unset.back() == before.back());
                if (eight) CHECK(unset.back() == fuse_cap(FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT, k.shape.n_traj / 8) && unset.back() >= before.back());
            }
            differ = differ || !same_plan(fuse_groups(rec, dead, lay, shape, unset, lanes, 1), fuse_groups(rec, dead, lay, shape, before, lanes, 1));
        }
        n_fused += any_fused;
        n_differ += differ;
    }
    std::printf("random captures: %d of 500 with a group of two or more under a named budget; %d whose plan under the defaults differs from the one budget of before\n", n_fused, n_differ);
    CHECK(2 * n_fused >= 500);    // otherwise the equalities hold vacuously
    CHECK(FUSE_WAVES_EIGHT_PER_WAVE_DEFAULT == FUSE_WAVES_DEFAULT || n_differ >= 50);

    if (failures == 0) std::printf("capture_kernel_budget OK\n");
    return failures == 0 ? 0 : 1;
}
