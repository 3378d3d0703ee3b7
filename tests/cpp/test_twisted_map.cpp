// CPU test of csrc/qp_twisted_map.h: the piece map of solve_twisted_kernel's copy-out in the latency shapes (16 lanes per trajectory:
// NSUB = 2, tiles of 4; 8 lanes per trajectory: NSUB = 1, tiles of 8), for every (r, M) of kernel_instances.h.  The header is included
// without the HIP runtime; the kernel reads the same functions.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "qp_twisted_map.h"

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

template <int nsub>
static void check_shape(int r, int M) {
    const int tile = nsub == 2 ? 4 : 8, nc = 2 * r, steps = twmap_steps<nsub>(M);
    const int mL = (M + 1) / 2, mR = M / 2;
    const long long tile_bytes = (long long)tile * 3 * M * nc * 8;
    std::vector<int> cover((size_t)(tile_bytes / 16), 0);

    // the row order: a bijection between rest and (trajectory, sub, side), and its inverse
    {
        std::vector<int> seen(16, 0);
        for (int tl = 0; tl < tile; ++tl)
            for (int sub = 0; sub < nsub; ++sub)
                for (int side = 0; side < 2; ++side) {
                    const int rest = twmap_rest<nsub>(tl, sub, side);
                    CHECK(rest >= 0 && rest < 16, "rest %d", rest);
                    if (rest < 0 || rest >= 16) continue;
                    ++seen[rest];
                    CHECK(twmap_rest_traj<nsub>(rest) == tl && twmap_rest_sub<nsub>(rest) == sub && twmap_rest_side<nsub>(rest) == side, "nsub %d rest %d", nsub, rest);
                }
        for (int i = 0; i < 16; ++i) CHECK(seen[i] == 1, "nsub %d: row %d used %d times", nsub, i, seen[i]);
    }

    for (int step = 0; step < steps; ++step)
        for (int axis = 0; axis < 3; ++axis) {
            TwistedPiece p[64];
            for (int lane = 0; lane < 64; ++lane) {
                p[lane] = twmap_piece<nsub>(lane, step, axis, M, r);
                const TwistedPiece& q = p[lane];
                // dropped: exactly the lanes whose producer has no segment in this step, and the padding column of a 48-byte chunk
                const int jv = step * nsub + q.sub, mside = q.side ? mR : mL;
                const bool expect_keep = jv < mside && q.col < r;
                CHECK(q.keep == expect_keep, "nsub %d r %d M %d step %d lane %d: keep %d", nsub, r, M, step, lane, (int)q.keep);
                CHECK(q.col == (lane & 3) && q.traj >= 0 && q.traj < tile && q.sub >= 0 && q.sub < nsub && (q.side == 0 || q.side == 1), "lane %d", lane);
                if (!q.keep) continue;
                // no kept piece outside the tile, every one at its (trajectory, axis, segment, column)
                CHECK(q.segment >= 0 && q.segment < M, "segment %d", q.segment);
                CHECK(q.segment == (q.side ? M - 1 - jv : jv), "segment %d of own %d", q.segment, jv);
                CHECK(q.byte >= 0 && q.byte + 16 <= tile_bytes && q.byte % 16 == 0, "byte %lld of %lld", q.byte, tile_bytes);
                CHECK(q.byte == ((((long long)q.traj * 3 + axis) * M + q.segment) * nc + 2 * q.col) * 8, "byte %lld", q.byte);
                if (q.byte >= 0 && q.byte + 16 <= tile_bytes) ++cover[(size_t)(q.byte / 16)];
            }
            if (nsub != 2) continue;
            const bool both = (step * 2 + 1 < mL) && (step * 2 + 1 < mR);   // both pairs of both sides have a segment in this step
            if (r == 4 && M % 2 == 0 && M >= 4) {
                if (both) {
                    // whole 128-byte lines, each from eight adjacent lanes in ascending address: 16 per instruction
                    for (int g = 0; g < 8; ++g)
                        for (int k = 0; k < 8; ++k) {
                            const TwistedPiece& q = p[g * 8 + k];
                            CHECK(q.keep, "M %d step %d lane %d dropped", M, step, g * 8 + k);
                            CHECK(p[g * 8].byte % 128 == 0 && q.byte == p[g * 8].byte + 16 * k, "M %d step %d lane %d: byte %lld, line at %lld", M, step, g * 8 + k, q.byte, p[g * 8].byte);
                        }
                } else {
                    // odd mL (M = 6, 10), last step: only pair 0 of each side has a segment, the two halves of the middle line (segments mL - 1 on
                    // side 0, mL on side 1), which no row order that keeps both sides ascending puts next to each other.  Nothing else is written.
                    CHECK(step == steps - 1 && mL % 2 == 1, "M %d step %d", M, step);
                    for (int lane = 0; lane < 64; ++lane)
                        if (p[lane].keep) CHECK(p[lane].sub == 0 && p[lane].segment == (p[lane].side ? mL : mL - 1), "M %d lane %d segment %d", M, lane, p[lane].segment);
                    // ... and the line is still whole within this one instruction: per trajectory the four lanes of (side 0, sub 0) write its
                    // first 64 bytes and the four lanes of (side 1, sub 0) its last 64, so the instruction writes 4 whole lines and nothing else
                    int kept = 0;
                    for (int lane = 0; lane < 64; ++lane) kept += p[lane].keep;
                    CHECK(kept == 32, "M %d step %d: %d pieces kept", M, step, kept);
                    for (int tl = 0; tl < tile; ++tl) {
                        const int l0 = twmap_rest<nsub>(tl, 0, 0) * 4, l1 = twmap_rest<nsub>(tl, 0, 1) * 4;
                        CHECK(p[l0].byte % 128 == 0, "M %d trajectory %d: line at %lld", M, tl, p[l0].byte);
                        for (int k = 0; k < 4; ++k) {
                            CHECK(p[l0 + k].keep && p[l0 + k].byte == p[l0].byte + 16 * k, "M %d trajectory %d first half, column %d", M, tl, k);
                            CHECK(p[l1 + k].keep && p[l1 + k].byte == p[l0].byte + 64 + 16 * k, "M %d trajectory %d second half, column %d", M, tl, k);
                        }
                    }
                }
            }
            if (r == 3) {
                // adjacent 48-byte chunks form one 96-byte run, copied by eight adjacent lanes (two of them padding) in ascending address
                for (int g = 0; g < 8; ++g) {
                    if (!(p[g * 8].keep && p[g * 8 + 4].keep)) continue;
                    for (int k = 0; k < 8; ++k) {
                        const TwistedPiece& q = p[g * 8 + k];
                        if ((k & 3) == 3) { CHECK(!q.keep, "padding column kept"); continue; }
                        CHECK(q.keep && q.byte == p[g * 8].byte + 48 * (k >> 2) + 16 * (k & 3), "r 3 M %d step %d lane %d: byte %lld, run at %lld", M, step, g * 8 + k, q.byte, p[g * 8].byte);
                    }
                }
                // ... and whenever both pairs of a side have a segment, that is the case
                if (both)
                    for (int g = 0; g < 8; ++g) CHECK(p[g * 8].keep && p[g * 8 + 4].keep, "r 3 M %d step %d group %d", M, step, g);
            }
        }
    // the kept pieces of all steps cover every (trajectory, axis) row exactly once
    for (size_t i = 0; i < cover.size(); ++i) CHECK(cover[i] == 1, "nsub %d r %d M %d: piece %zu written %d times", nsub, r, M, i, cover[i]);
}

int main() {
    for (int M : R4_M) { check_shape<1>(4, M); check_shape<2>(4, M); }
    for (int M : R3_M) { check_shape<1>(3, M); check_shape<2>(3, M); }
    // the headline shape: 2 steps x 3 instructions of 16 whole lines, every byte once (checked above); its first instruction spelled out
    {
        const TwistedPiece a = twmap_piece<2>(0, 0, 0, 8, 4), b = twmap_piece<2>(4, 0, 0, 8, 4), c = twmap_piece<2>(8, 0, 0, 8, 4), d = twmap_piece<2>(12, 0, 0, 8, 4);
        CHECK(a.segment == 0 && b.segment == 1 && c.segment == 6 && d.segment == 7, "segments %d %d %d %d", a.segment, b.segment, c.segment, d.segment);
        CHECK(a.side == 0 && b.side == 0 && c.side == 1 && d.side == 1 && a.sub == 0 && b.sub == 1 && c.sub == 1 && d.sub == 0, "row order");
        const TwistedPiece e = twmap_piece<2>(0, 1, 0, 8, 4), f = twmap_piece<2>(12, 1, 0, 8, 4);
        CHECK(e.segment == 2 && f.segment == 5, "step 1: %d %d", e.segment, f.segment);
    }
    if (g_fail) { printf("twisted_map: %d checks FAILED\n", g_fail); return 1; }
    printf("twisted_map OK\n");
    return 0;
}
