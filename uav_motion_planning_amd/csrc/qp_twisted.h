// qp_twisted.h -- register-resident specialised kernel for uniform batches (compile-time R, M).
//
// Two lanes per trajectory ("twisted" / two-sided block elimination): lane L works in the original
// time direction on segments 0..mL-1, lane R on the time-reversed trajectory (segments M-1..mL), both
// eliminating interior knots towards the meeting knot c = mL with the SAME instruction stream -- the
// min-control problem is time-reversal symmetric (derivative d picks up (-1)^d).  At the meeting knot
// the two partial Schur complements are exchanged through DPP (lane ^ 1), both lanes solve it, then
// back-substitute their own half and emit the monomial coefficients of their own segments.
//
// Memory plan (one wave = one workgroup = TILE trajectories per tile, persistent over tiles):
//   * inputs of tile n+1 are prefetched HBM -> LDS by LDS-DMA (global_load_lds_dwordx4, no VGPRs)
//     while tile n is being eliminated: double-buffered 2 x 13.25 KiB (r=4, M=8);
//   * all per-knot state (E_k, h_k) lives in VGPRs -- nothing is spilled to HBM;
//   * coefficients of one segment (3 axes) are transposed through LDS so that every
//     global_store_dwordx4 writes whole 2r-coefficient chunks from adjacent lanes.
// HBM traffic is therefore exactly the algorithmic bytes.
#pragma once
#include <type_traits>

#include "qp_core_kernels.h"
#include "qp_twisted_map.h"
#include "qp_twisted_map8.h"
#include "qp_wave_utils.h"

#ifndef UAVQP_STAMP   // (probe builds under tools/ubench define their own: per-wave timelines)
#ifdef UAVQP_PHASE_TIMING
#define UAVQP_STAMP(i) do { if (a.stamps && blockIdx.x == 0 && threadIdx.x == 0) a.stamps[i] = __builtin_readcyclecounter(); } while (0)
#else
#define UAVQP_STAMP(i) do {} while (0)
#endif
#endif

namespace uavqp {

template <int R, int M, int TILE, int LPT = 2>
struct TwistedCfg {
    static constexpr int ND = R - 1, NC = 2 * R, NK = M + 1;
    static constexpr int mL = (M + 1) / 2, mR = M / 2;
    static constexpr int WP_D = TILE * NK * 3;  // doubles per tile
    static constexpr int T_D = TILE * M;
    static constexpr int BC_D = TILE * 2 * ND * 3;
    static constexpr int T_OFF = WP_D, BC_OFF = WP_D + T_D;
    static constexpr int IN_D = WP_D + T_D + BC_D;
    static constexpr int PQ = NC / 2;  // 16-byte pieces per chunk
    // LPT = lanes per trajectory.  2: one (L, R) lane pair carries all three axes (throughput shape).
    // 8: one lane pair per axis (+ one idle pair) -- the matrix elimination is repeated by the three pairs,
    // right-hand sides, back-substitution and coefficient emission are split by axis (latency shape for
    // small batches: ~2x shorter critical path per wave, 8 trajectories per wave).
    static constexpr int NAX = LPT == 2 ? 3 : 1;
    // Emission chunk: CH own segments of one axis per unit (r = 4: 2 segments = one 128-B line; r = 3: 4
    // segments = 192 B).  Staging = 64 lane rows of CH*NC doubles, row stride 4 (mod 8) dwords for
    // conflict-free ds_write_b128.  If double-buffered input + staging exceed the LDS budget of 4 waves
    // per CU (40448 B each), the staging rows alias the current input buffer instead.
    static constexpr int CH = (NC * 8) % 64 == 0 ? 2 : 4;
    static constexpr int STAGE_STRIDE0 = CH * NC + 2;
    static constexpr int STAGE_STRIDE = (STAGE_STRIDE0 * 2) % 8 == 4 ? STAGE_STRIDE0 : STAGE_STRIDE0 + 2;
    static constexpr int STAGE_D = 64 * STAGE_STRIDE;
    // (measured, 1 M batch: aliasing wins for r = 3 -- (3,16) 3.85 vs 3.71, (3,12) 3.97 vs 3.43 TB/s -- but the
    // register cost of the pre-loaded positions spills for r = 4, M = 12: 3.46 vs 3.92 TB/s with 3 waves/CU)
    static constexpr bool ALIAS = LPT == 2 && R == 3 && (2 * IN_D + STAGE_D) * 8 > 40448;
    // LPT >= 8 (latency shapes): every emission step leaves one NC-double chunk per working lane (6 * LPT / 8 per trajectory:
    // TILE * 6 * LPT / 8 = 48 rows for both shapes) in an LDS row of stride 10 doubles (20 dwords: the b128 writes of 16 rows tile
    // the 64 banks), read back linearly by the wave for the software-pipelined copy-out; rows 48.. take the writes of the idle pairs.
    static constexpr int ROWS8 = LPT >= 8 ? TILE * 6 * (LPT / 8) : 0, RS8 = 10;
    static_assert(LPT < 8 || ROWS8 == 48, "the copy-out maps 3 axes x 16 rows");
    static constexpr int OUT_D = LPT >= 8 ? (ROWS8 + 16) * RS8 + 16 : ((LPT == 2 && !ALIAS) ? STAGE_D : 2);
    // solve_twisted_group8_kernel (eight trajectories per wave, both segments of a step per lane pair): six blocks of 16 rows and 16 rows
    // behind them for the writes of the idle pairs, laid out by qp_twisted_map8.h.
    // Three waves per SIMD are twelve workgroups per CU, nominally a twelfth of its 160 KiB of LDS each.  Where the input tile and the
    // whole staging area are more than that ((3, 16) alone: 14336 bytes) the idle pairs do not write and their 16 rows are not allocated
    // (13056 bytes): the six blocks end below TWMAP8_IDLE_BASE, and every other shape keeps its unpredicated writes.
    // NOMINALLY: the figure counts bytes as declared.  The granule in which the hardware allocates LDS to a workgroup was not
    // established here; if it is the 1280 bytes (320 dwords) that 160 KiB over a 7-bit block count suggest, 13056 and (3, 12)'s 13312
    // both round to 14080 and a CU holds eleven such workgroups (ten of 14336), twelve only up to 12800 bytes -- (4, 8) has 12672.
    // What this case buys (3, 16) is then the eleventh workgroup, not the twelfth; no timing tells the two apart (measurement log).
    static constexpr bool IDLE_ROWS2 = (IN_D + TWMAP8_STAGE_DOUBLES) * 8 * 12 <= 160 * 1024;
    static constexpr int OUT2_D = IDLE_ROWS2 ? TWMAP8_STAGE_DOUBLES : TWMAP8_IDLE_BASE;
    static_assert(twmap8_row_addr(TWMAP8_PIECES - 1, 15) + TWMAP8_ROW_STRIDE <= TWMAP8_IDLE_BASE, "the blocks end in front of the idle rows");
    static_assert(RS8 == TWMAP8_ROW_STRIDE, "one row stride for the latency shapes");
    static_assert(!ALIAS || STAGE_D <= IN_D, "aliased staging rows must fit the input buffer");
    static_assert(WP_D % 2 == 0 && T_D % 2 == 0 && BC_D % 2 == 0, "tile arrays must be whole 16-B pairs");
};

// ONE (latency shapes): the launch has exactly one WHOLE tile per wave (grid == n_tiles, n_traj % TILE == 0 -- the host checks both):
// no shifted or guarded tile, no prefetch and no second input buffer, nothing that depends on the batch size; the tile loop makes one trip.
// (It must stay that way: the ONE instantiation never reads n_traj, and tools/ubench/twisted_phases.hip passes the timeline slab of a
// back-to-back launch in that argument.  Every use of a.n_traj below sits behind an `ONE ?` / `if constexpr (ONE)`.)
//
// Arguments: FLAT, one signature for every tile shape, the three arrays the LDS-DMA needs in front.  The translation units of this kernel
// are compiled with the leading six arguments preloaded into SGPRs at wave launch (csrc/Makefile: TWISTED_FLAGS; a struct passed by
// value is never preloaded): a wave issues its input loads without first fetching pointers from the kernarg segment, which is a fresh,
// scalar-cache-cold address for every launch.  The host marshals them in one place: TwistedParams (uavqp.hip).
#ifdef UAVQP_PHASE_TIMING
#define UAVQP_TWISTED_STAMPS_PARAM , long long* stamps
#define UAVQP_TWISTED_STAMPS_INIT , stamps
#else
#define UAVQP_TWISTED_STAMPS_PARAM
#define UAVQP_TWISTED_STAMPS_INIT
#endif
#define UAVQP_TWISTED_SIG const double*, const double*, const double*, double*, int32_t*, int UAVQP_TWISTED_STAMPS_PARAM
struct TwistedArgs {   // what the body (qp_twisted_body.h) reads: the kernel's own arguments under the names they had in BatchArgs
    const double* waypoints;
    const double* times;
    const double* bc;
    double* coeff;
    int32_t* status;
    int n_traj;
#ifdef UAVQP_PHASE_TIMING
    long long* stamps;
#endif
};
constexpr bool twmap_plain_rows() {   // qp_twisted_map.h with one lane pair per axis is the plain decode the 8-lane shape spells out
    for (int rest = 0; rest < 16; ++rest)
        if (twmap_rest_side<1>(rest) != (rest & 1) || twmap_rest_sub<1>(rest) != 0 || twmap_rest_traj<1>(rest) != rest >> 1) return false;
    return true;
}
template <int R, int M, int TILE, int LPT = 2, bool ONE = false>
__global__ __launch_bounds__(64, 1) void solve_twisted_kernel(const double* waypoints, const double* times, const double* bc, double* coeff,
                                                              int32_t* status, int n_traj UAVQP_TWISTED_STAMPS_PARAM) {
    const TwistedArgs a{waypoints, times, bc, coeff, status, n_traj UAVQP_TWISTED_STAMPS_INIT};
    constexpr bool EMIT2 = false;
#include "qp_twisted_body.h"
}

// Several independent solves of ONE shape in one launch (uavqp_capture.h: fuse_groups; built by uavqp_capture_end only, never launched
// eagerly).  Grid (n_tiles, F): blockIdx.y picks one of up to GROUP_MAX pointer sets, blockIdx.x the tile; the wave then runs the ONE path
// of solve_twisted_kernel -- the same statements (qp_twisted_body.h), hence the same arithmetic: a replay stays bitwise equal to eager order.  The sets travel BY
// VALUE in the kernarg segment, so there is no device table whose lifetime a graph would have to own; a struct by value is not preloaded
// into SGPRs, so this kernel's waves fetch their five pointers (scalar loads, offset by blockIdx.y) before they issue their input loads:
// accepted here, because up to three co-resident waves of a SIMD cover each other's latencies, which a launch of one solve never has.
// n_traj is never read on the ONE path; it is passed as 0.
static constexpr int GROUP_MAX = 8;
struct TwistedGroupSet {
    const double* waypoints;
    const double* times;
    const double* bc;
    double* coeff;
    int32_t* status;   // null: no status array, or a store that a later solve overwrites (dead_status_stores)
};
struct TwistedGroupArgs {
    TwistedGroupSet set[GROUP_MAX];
};
#define UAVQP_TWISTED_GROUP_SIG const uavqp::TwistedGroupArgs
template <int R, int M, int TILE, int LPT>
__global__ __launch_bounds__(64, 1) void solve_twisted_group_kernel(const TwistedGroupArgs group) {
    static_assert(LPT >= 8, "groups are built from launches of one whole tile per wave: latency shapes only");
    constexpr bool ONE = true;
    const TwistedGroupSet& mine = group.set[blockIdx.y];
#ifdef UAVQP_PHASE_TIMING
    const TwistedArgs a{mine.waypoints, mine.times, mine.bc, mine.coeff, mine.status, 0, nullptr};
#else
    const TwistedArgs a{mine.waypoints, mine.times, mine.bc, mine.coeff, mine.status, 0};
#endif
    constexpr bool EMIT2 = false;
#include "qp_twisted_body.h"
}

// The group of 16-lane solves once more, with EIGHT trajectories per wave: what uavqp_capture_end puts into a group of two or more tile-4
// launches whose batch is a whole number of eights (uavqp_capture.h: group_kernel_choice).  The 16-lane shape gives every (trajectory,
// axis, side) two lane pairs that both run elimination, meeting knot and back-substitution and split only the emission: latency for an
// isolated launch, where a SIMD holds one wave -- and pure cost in a fused replay, whose SIMDs are full.  Here a wave is laid out as the
// 8-lane shape (one pair per (trajectory, axis)), runs those statements once, and then emits BOTH segments of every step with the 16-lane
// shape's arithmetic (qp_twisted_body.h, EMIT2: segment_coeffs on the reloaded duration, not the 8-lane shape's kept inverse powers):
// per (trajectory, axis, side, segment) the operations of solve_twisted_kernel<R, M, 4, 16, true>, so a replay stays bitwise equal to
// eager order.  Grid (n_traj / 8, members), block 64; the copy-out map is qp_twisted_map8.h.
// Every instantiation fits three waves per SIMD -- at most 168 VGPRs, no scratch, in declared bytes at most a twelfth of a CU's LDS
// (tests/test_twisted_group8_three_waves.py; TwistedCfg::IDLE_ROWS2 on the allocation granule) -- since the copy-out decode starts from an opaque copy of the lane index and is computed
// behind the elimination instead of being hoisted in front of the load wait (qp_twisted_body.h, EMIT2).  VGPRs, waves per SIMD:
//   r = 4:  M = 2  62, 4   3  130, 3   4  98, 4   5  152, 3   6  126, 4   8  156, 3                        (before: 6  156, 3   8  182, 2)
//   r = 3:  M = 2  52, 4   3  86, 4   4  66, 4   5  97, 4   6  84, 4   7  108, 4   8  96, 4   10  110, 3 and 12  124, 3 (by LDS)   16  154, 3
//                                                                                                          (before: 16  226, 2)
#define UAVQP_TWISTED_GROUP8_SIG const uavqp::TwistedGroupArgs
template <int R, int M>
__global__ __launch_bounds__(64, 1) void solve_twisted_group8_kernel(const TwistedGroupArgs group) {
    constexpr int TILE = TWMAP8_TILE, LPT = 8;
    constexpr bool ONE = true, EMIT2 = true;
    const TwistedGroupSet& mine = group.set[blockIdx.y];
#ifdef UAVQP_PHASE_TIMING
    const TwistedArgs a{mine.waypoints, mine.times, mine.bc, mine.coeff, mine.status, 0, nullptr};
#else
    const TwistedArgs a{mine.waypoints, mine.times, mine.bc, mine.coeff, mine.status, 0};
#endif
#include "qp_twisted_body.h"
}

}  // namespace uavqp
