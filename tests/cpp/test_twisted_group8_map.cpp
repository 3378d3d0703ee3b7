// CPU test of csrc/qp_twisted_map8.h -- the piece map of solve_twisted_group8_kernel's copy-out (eight trajectories per wave, both segments
// of a 16-lane step per lane pair, six stores per lane and step) -- for all 20 (r, M) of kernel_instances.h, and of the host rule that
// decides which kernel a group's node gets (csrc/uavqp_capture.h: group_kernel_choice).  Both headers are included without the HIP
// runtime; the kernel and uavqp_capture_end read the same functions.
// With arguments "choose members r M tile n_traj num_cus" the program prints that rule's answer for a group of captured launches of
// uavqp_solve_batch_device (0 = as captured, 1 = the group kernel of the launches' own tile, 2 = eight trajectories per wave):
// tests/test_gpu_twisted_group8.py asks it which kernel its captures ran.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernel_instances.h"
#include "qp_twisted_map8.h"
#include "uavqp_capture.h"

using namespace uavqp;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (g_fail < 20) { printf("FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
            ++g_fail;                                      \
        }                                                  \
    } while (0)

static const int R4_M[] = {2, 3, 4, 5, 6, 7, 8, 9, 10, 12};
static const int R3_M[] = {2, 3, 4, 5, 6, 7, 8, 10, 12, 16};

// the launch of uavqp_solve_batch_device as far as grouping goes (uavqp.hip: the tile rule; tests/cpp/capture_fuse_plan.cpp has the same lines)
static int choose(int members, int r, int M, int tile, int n_traj, int num_cus) {
    const int n_tiles = (n_traj + tile - 1) / tile, max_wg = num_cus * 4;
    const int grid = n_tiles < max_wg ? n_tiles : max_wg;
    const bool one = grid == n_tiles && n_traj % tile == 0 && uavqp_twisted_group_exists(r, M, tile);
    return (int)uavqp_capture::group_kernel_choice(members, tile, one, n_traj, uavqp_twisted_group8_exists(r, M));
}

static void check_shape(int r, int M) {
    const int tile = TWMAP8_TILE, nc = 2 * r, steps = twmap8_steps(M);
    const int mL = (M + 1) / 2, mR = M / 2;
    const long long tile_bytes = (long long)tile * 3 * M * nc * 8;
    std::vector<int> cover((size_t)(tile_bytes / 16), 0);
    CHECK(steps == (mL + 1) / 2, "steps %d", steps);

    // the staging rows: a bijection between 0 .. 95 and (trajectory, axis, side, sub); the producing lanes are the 48 working lanes
    {
        std::vector<int> seen(TWMAP8_ROWS, 0), lanes(64, 0);
        for (int tl = 0; tl < tile; ++tl)
            for (int axis = 0; axis < 3; ++axis)
                for (int side = 0; side < 2; ++side) {
                    const int lane = twmap8_lane(tl, axis, side);
                    CHECK(lane >= 0 && lane < 64 && lane / 8 == tl && ((lane % 8) >> 1) == axis && (lane & 1) == side, "lane %d", lane);
                    if (lane >= 0 && lane < 64) ++lanes[lane];
                    for (int sub = 0; sub < 2; ++sub) {
                        const int row = twmap8_row(tl, axis, side, sub);
                        CHECK(row >= 0 && row < TWMAP8_ROWS, "row %d", row);
                        if (row < 0 || row >= TWMAP8_ROWS) continue;
                        ++seen[row];
                        CHECK(row / 16 == twmap8_block(tl, axis) && twmap8_block_half(row / 16) == tl / 4 && twmap8_block_axis(row / 16) == axis, "row %d", row);
                    }
                }
        for (int i = 0; i < TWMAP8_ROWS; ++i) CHECK(seen[i] == 1, "row %d used %d times", i, seen[i]);
        int working = 0;
        for (int i = 0; i < 64; ++i) { CHECK(lanes[i] <= 1, "lane %d", i); working += lanes[i]; }
        CHECK(working == 48, "%d working lanes", working);
    }

    for (int step = 0; step < steps; ++step)
        for (int piece = 0; piece < TWMAP8_PIECES; ++piece) {
            TwistedPiece8 p[64];
            for (int lane = 0; lane < 64; ++lane) {
                p[lane] = twmap8_piece(lane, step, piece, M, r);
                const TwistedPiece8& q = p[lane];
                // dropped: exactly the pieces whose producer has no such segment, and the padding column of a 48-byte chunk
                const int jv = step * 2 + q.sub, mside = q.side ? mR : mL;
                const bool expect_keep = jv < mside && q.col < r;
                CHECK(q.keep == expect_keep, "r %d M %d step %d piece %d lane %d: keep %d", r, M, step, piece, lane, (int)q.keep);
                CHECK(q.col == (lane & 3) && q.traj >= 0 && q.traj < tile && (q.sub == 0 || q.sub == 1) && (q.side == 0 || q.side == 1) && q.axis >= 0 && q.axis < 3, "lane %d", lane);
                // read from the row its producer wrote
                CHECK(q.row == twmap8_row(q.traj, q.axis, q.side, q.sub), "r %d M %d piece %d lane %d: row %d", r, M, piece, lane, q.row);
                if (!q.keep) continue;
                CHECK(q.segment >= 0 && q.segment < M, "segment %d", q.segment);
                CHECK(q.segment == (q.side ? M - 1 - jv : jv), "segment %d of own %d", q.segment, jv);
                CHECK(q.byte >= 0 && q.byte + 16 <= tile_bytes && q.byte % 16 == 0, "byte %lld of %lld", q.byte, tile_bytes);
                CHECK(q.byte == ((((long long)q.traj * 3 + q.axis) * M + q.segment) * nc + 2 * q.col) * 8, "byte %lld", q.byte);
                if (q.byte >= 0 && q.byte + 16 <= tile_bytes) ++cover[(size_t)(q.byte / 16)];
            }
            // one instruction is the 16-lane kernel's store of one axis of four trajectories: the same map, shifted by the half
            for (int lane = 0; lane < 64; ++lane) {
                const TwistedPiece o = twmap_piece<2>(lane, step, twmap8_block_axis(piece), M, r);
                const TwistedPiece8& q = p[lane];
                CHECK(o.keep == q.keep && o.traj + 4 * twmap8_block_half(piece) == q.traj && o.side == q.side && o.sub == q.sub && o.segment == q.segment && o.col == q.col,
                      "r %d M %d step %d piece %d lane %d differs from the 16-lane map", r, M, step, piece, lane);
                if (q.keep) CHECK(q.byte == o.byte + (long long)twmap8_block_half(piece) * 4 * 3 * M * nc * 8, "byte %lld", q.byte);
            }
            const bool both = (step * 2 + 1 < mL) && (step * 2 + 1 < mR);   // both sides have both segments of this step
            if (r == 4 && M % 2 == 0 && M >= 4) {
                if (both) {
                    // whole 128-byte lines, each from eight adjacent lanes in ascending address: 16 per instruction
                    for (int g = 0; g < 8; ++g)
                        for (int k = 0; k < 8; ++k) {
                            const TwistedPiece8& q = p[g * 8 + k];
                            CHECK(q.keep, "M %d step %d lane %d dropped", M, step, g * 8 + k);
                            CHECK(p[g * 8].byte % 128 == 0 && q.byte == p[g * 8].byte + 16 * k, "M %d step %d lane %d: byte %lld, line at %lld", M, step, g * 8 + k, q.byte, p[g * 8].byte);
                        }
                } else {
                    // odd mL (M = 6, 10), last step: the two halves of the middle line of every (trajectory, axis), whole within the instruction
                    CHECK(step == steps - 1 && mL % 2 == 1, "M %d step %d", M, step);
                    int kept = 0;
                    for (int lane = 0; lane < 64; ++lane) {
                        kept += p[lane].keep;
                        if (p[lane].keep) CHECK(p[lane].sub == 0 && p[lane].segment == (p[lane].side ? mL : mL - 1), "M %d lane %d segment %d", M, lane, p[lane].segment);
                    }
                    CHECK(kept == 32, "M %d step %d: %d pieces kept", M, step, kept);
                    for (int t4 = 0; t4 < 4; ++t4) {
                        const int l0 = twmap_rest<2>(t4, 0, 0) * 4, l1 = twmap_rest<2>(t4, 0, 1) * 4;
                        CHECK(p[l0].byte % 128 == 0, "M %d trajectory %d: line at %lld", M, t4, p[l0].byte);
                        for (int k = 0; k < 4; ++k) {
                            CHECK(p[l0 + k].keep && p[l0 + k].byte == p[l0].byte + 16 * k, "M %d trajectory %d first half, column %d", M, t4, k);
                            CHECK(p[l1 + k].keep && p[l1 + k].byte == p[l0].byte + 64 + 16 * k, "M %d trajectory %d second half, column %d", M, t4, k);
                        }
                    }
                }
            }
            if (r == 3 && both)   // adjacent 48-byte chunks form one 96-byte run, copied by eight adjacent lanes (two of them padding)
                for (int g = 0; g < 8; ++g)
                    for (int k = 0; k < 8; ++k) {
                        const TwistedPiece8& q = p[g * 8 + k];
                        if ((k & 3) == 3) { CHECK(!q.keep, "padding column kept"); continue; }
                        CHECK(q.keep && q.byte == p[g * 8].byte + 48 * (k >> 2) + 16 * (k & 3), "r 3 M %d step %d lane %d: byte %lld, run at %lld", M, step, g * 8 + k, q.byte, p[g * 8].byte);
                    }
        }
    // the kept pieces of all steps cover every coefficient of the eight trajectories exactly once
    for (size_t i = 0; i < cover.size(); ++i) CHECK(cover[i] == 1, "r %d M %d: piece %zu written %d times", r, M, i, cover[i]);
}

// the staging rows in LDS: no two overlap (a row is up to 8 doubles), all inside the staging area and 16-byte aligned, linear in `rest`
// within a block (the copy-out reads them so)
static void check_lds() {
    std::vector<int> owner((size_t)TWMAP8_STAGE_DOUBLES, -1);
    int id = 0;
    auto claim = [&](int addr) {
        CHECK(addr >= 0 && addr % 2 == 0 && addr + TWMAP8_ROW_DOUBLES <= TWMAP8_STAGE_DOUBLES, "row at %d", addr);
        for (int k = 0; k < TWMAP8_ROW_DOUBLES; ++k) {
            if (addr + k < 0 || addr + k >= TWMAP8_STAGE_DOUBLES) continue;
            CHECK(owner[(size_t)(addr + k)] == -1, "double %d is in rows %d and %d", addr + k, owner[(size_t)(addr + k)], id);
            owner[(size_t)(addr + k)] = id;
        }
        ++id;
    };
    for (int block = 0; block < TWMAP8_PIECES; ++block)
        for (int rest = 0; rest < 16; ++rest) {
            claim(twmap8_row_addr(block, rest));
            CHECK(twmap8_row_addr(block, rest) == twmap8_row_addr(block, 0) + rest * TWMAP8_ROW_STRIDE, "block %d row %d", block, rest);
        }
    for (int i = 0; i < 16; ++i) claim(twmap8_idle_addr(i));
    CHECK(id == TWMAP8_ROWS + 16, "%d rows", id);
    // the twelve b128 writes of 16 consecutive lanes (two trajectories x three axes x two sides, one sub) start in twelve different bank quads
    for (int group = 0; group < 4; ++group)
        for (int sub = 0; sub < 2; ++sub) {
            int used[16] = {};
            for (int l = 0; l < 16; ++l) {
                const int lane = group * 16 + l, tl = lane / 8, axis = (lane % 8) >> 1, side = lane & 1;
                if (axis == 3) continue;
                const int quad = (twmap8_row_addr(twmap8_block(tl, axis), twmap8_rest(tl, sub, side)) / 2) % 16;
                CHECK(used[quad] == 0, "lanes %d.., sub %d: bank quad %d twice", group * 16, sub, quad);
                ++used[quad];
            }
        }
}

static void check_choice() {
    using namespace uavqp_capture;
    const int cus = 256;
    for (int r = 3; r <= 4; ++r)
        for (int M : (r == 4 ? R4_M : R3_M)) {
            const bool g4 = uavqp_twisted_group_exists(r, M, 4), g8 = uavqp_twisted_group_exists(r, M, 8), w8 = uavqp_twisted_group8_exists(r, M);
            CHECK(!w8 || g4, "r %d M %d: an eight-per-wave kernel only where the tile-4 group kernel is", r, M);
            for (int members = 1; members <= FUSE_MAX; ++members)
                for (int n = 1; n <= 64; ++n) {
                    const int c4 = choose(members, r, M, 4, n, cus), c8 = choose(members, r, M, 8, n, cus);
                    if (members == 1) CHECK(c4 == GROUP_AS_CAPTURED && c8 == GROUP_AS_CAPTURED, "a group of one is the launch as captured");
                    if (members >= 2 && n % 8 != 0) CHECK(c4 == (g4 && n % 4 == 0 ? GROUP_OWN_TILE : GROUP_AS_CAPTURED), "r %d M %d n %d: %d", r, M, n, c4);
                    if (members >= 2 && n % 8 == 0) CHECK(c4 == (w8 ? GROUP_EIGHT_PER_WAVE : (g4 ? GROUP_OWN_TILE : GROUP_AS_CAPTURED)), "r %d M %d n %d: %d", r, M, n, c4);
                    // a launch at tile 8 never reaches the new kernel: its own group kernel, or none
                    CHECK(c8 == (members >= 2 && g8 && n % 8 == 0 ? GROUP_OWN_TILE : GROUP_AS_CAPTURED), "r %d M %d n %d at tile 8: %d", r, M, n, c8);
                }
        }
    // the pins of the existing yardsticks
    CHECK(!uavqp_twisted_group_exists(4, 8, 8), "(4, 8) at tile 8 has no group");
    CHECK(choose(8, 4, 8, 8, 4096, cus) == GROUP_AS_CAPTURED, "(4, 8) launched at tile 8 replays unfused");
    CHECK(uavqp_twisted_group8_exists(4, 8) && choose(2, 4, 8, 4, 4096, cus) == GROUP_EIGHT_PER_WAVE, "the headline: 4096 x (4, 8) at tile 4");
    CHECK(choose(2, 4, 8, 4, 4100, cus) == GROUP_AS_CAPTURED && choose(2, 4, 8, 4, 4092, cus) == GROUP_OWN_TILE, "no whole number of eights");
    CHECK(choose(2, 4, 8, 4, 8192, cus) == GROUP_AS_CAPTURED, "more tiles than waves: the kernel with the tile loop, no group");
    // the function itself, argument by argument
    CHECK(group_kernel_choice(1, 4, true, 4096, true) == GROUP_AS_CAPTURED && group_kernel_choice(2, 4, false, 4096, true) == GROUP_AS_CAPTURED, "one member / not `one`");
    CHECK(group_kernel_choice(2, 4, true, 4096, false) == GROUP_OWN_TILE && group_kernel_choice(2, 8, true, 4096, true) == GROUP_OWN_TILE, "no kernel / tile 8");
    CHECK(group_kernel_choice(2, 4, true, 12, true) == GROUP_OWN_TILE && group_kernel_choice(2, 4, true, 0, true) == GROUP_OWN_TILE, "n %% 8");
    CHECK(group_kernel_choice(8, 4, true, 8, true) == GROUP_EIGHT_PER_WAVE, "one wave");
}

int main(int argc, char** argv) {
    if (argc == 8 && std::strcmp(argv[1], "choose") == 0) {
        printf("%d\n", choose(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7])));
        return 0;
    }
    for (int M : R4_M) check_shape(4, M);
    for (int M : R3_M) check_shape(3, M);
    check_lds();
    check_choice();
    // the headline shape: 2 steps x 6 instructions of 16 whole lines; the first and the fourth instruction spelled out
    {
        const TwistedPiece8 a = twmap8_piece(0, 0, 0, 8, 4), b = twmap8_piece(4, 0, 0, 8, 4), c = twmap8_piece(8, 0, 0, 8, 4), d = twmap8_piece(12, 0, 0, 8, 4);
        CHECK(a.segment == 0 && b.segment == 1 && c.segment == 6 && d.segment == 7 && a.traj == 0 && d.traj == 0 && a.axis == 0, "segments %d %d %d %d", a.segment, b.segment, c.segment, d.segment);
        const TwistedPiece8 e = twmap8_piece(16, 1, 3, 8, 4), f = twmap8_piece(63, 1, 5, 8, 4);
        CHECK(e.traj == 5 && e.axis == 0 && e.segment == 2 && f.traj == 7 && f.axis == 2 && f.segment == 5 && f.col == 3, "second half: %d %d %d, %d %d %d", e.traj, e.axis, e.segment, f.traj, f.axis, f.segment);
    }
    if (g_fail) { printf("twisted_group8_map: %d checks FAILED\n", g_fail); return 1; }
    printf("twisted_group8_map OK\n");
    return 0;
}
