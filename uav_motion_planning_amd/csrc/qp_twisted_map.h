// qp_twisted_map.h -- which 16-byte piece of the coefficient array every lane of solve_twisted_kernel's latency shapes (qp_twisted.h,
// LPT >= 8) copies out in every emission step, as plain integer functions.  No state; compiles without the HIP runtime too: the kernel
// and tests/cpp/test_twisted_map.cpp read the same code.
//
// Producers.  NSUB = LPT / 8 lane pairs per (trajectory, axis); pair `sub` of side `side` (0 = original direction, 1 = reversed) emits
// its OWN segment step * NSUB + sub in step `step` -- global segment jv on side 0, M - 1 - jv on side 1 -- while it has one
// (jv < mL = (M + 1) / 2 on side 0, jv < mR = M / 2 on side 1).  With NSUB = 2 the two pairs of a side emit ADJACENT segments in the
// same step: for r = 4 (64-byte chunks) and even M that is one whole 128-byte line per (trajectory, axis, side) and step.
//
// Staging rows.  One LDS row per (trajectory, sub, side) and axis; the row index without the axis is `rest`.  The copy-out reads the
// rows linearly, four 16-byte columns per row (lane = rest * 4 + column), so the rows of a trajectory are ordered by ASCENDING ADDRESS
// of what they hold: side 0 sub 0, side 0 sub 1, side 1 sub 1, side 1 sub 0 (the reversed lanes' segments descend with sub).  The eight
// lanes rest = 2 i, 2 i + 1 then copy the two chunks of a line, in address order.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define UAVQP_MAP_HD __host__ __device__
#else
#define UAVQP_MAP_HD
#endif

namespace uavqp {

// emission steps of a wave: own segments of the longer side, NSUB per step
template <int nsub>
UAVQP_MAP_HD constexpr int twmap_steps(int M) { return ((M + 1) / 2 + nsub - 1) / nsub; }
// own segment that pair `sub` emits in step `step`
template <int nsub>
UAVQP_MAP_HD constexpr int twmap_own_segment(int step, int sub) { return step * nsub + sub; }
// own segments of a side
UAVQP_MAP_HD constexpr int twmap_side_segments(int M, int side) { return side ? M / 2 : (M + 1) / 2; }
// global segment of own segment jv
UAVQP_MAP_HD constexpr int twmap_global_segment(int M, int side, int jv) { return side ? M - 1 - jv : jv; }
// staging row (without the axis) of the producer (trajectory of the tile, sub, side)
template <int nsub>
UAVQP_MAP_HD constexpr int twmap_rest(int tl, int sub, int side) { return nsub == 2 ? tl * 4 + side * 2 + (sub ^ side) : tl * 2 + side; }
// ... and back
template <int nsub>
UAVQP_MAP_HD constexpr int twmap_rest_traj(int rest) { return rest >> nsub; }
template <int nsub>
UAVQP_MAP_HD constexpr int twmap_rest_side(int rest) { return nsub == 2 ? (rest >> 1) & 1 : rest & 1; }
template <int nsub>
UAVQP_MAP_HD constexpr int twmap_rest_sub(int rest) { return nsub == 2 ? (rest ^ (rest >> 1)) & 1 : 0; }

// The piece lane `lane` copies in step `step` with copy instruction `axis` (one instruction per axis), for a tile of whole trajectories.
struct TwistedPiece {
    int traj, side, sub;   // producer: trajectory of the tile, side, lane pair
    int segment;           // global segment
    int col;               // 16-byte column of the 2r-coefficient chunk
    bool keep;             // false: the producer has no segment in this step, or the column is padding (r = 3) -- the store is dropped
    long long byte;        // offset in the tile's coefficients [traj][axis][segment][2r] of doubles; meaningful if keep
};
template <int nsub>
UAVQP_MAP_HD inline TwistedPiece twmap_piece(int lane, int step, int axis, int M, int r) {
    const int rest = lane >> 2, nc = 2 * r;
    TwistedPiece p;
    p.col = lane & 3;
    p.traj = twmap_rest_traj<nsub>(rest);
    p.side = twmap_rest_side<nsub>(rest);
    p.sub = twmap_rest_sub<nsub>(rest);
    const int jv = twmap_own_segment<nsub>(step, p.sub);
    p.segment = twmap_global_segment(M, p.side, jv);
    p.keep = p.col < nc / 2 && jv < twmap_side_segments(M, p.side);
    p.byte = ((((long long)p.traj * 3 + axis) * M + p.segment) * nc + 2 * p.col) * 8;
    return p;
}

}  // namespace uavqp
