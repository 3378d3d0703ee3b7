// qp_twisted_map8.h -- which 16-byte piece of the coefficient array every lane of solve_twisted_group8_kernel (qp_twisted.h) copies out in
// every emission step, as plain integer functions, next to qp_twisted_map.h and in its terms.  No state; compiles without the HIP runtime
// too: the kernel and tests/cpp/test_twisted_group8_map.cpp read the same code.
//
// The wave holds EIGHT trajectories, one lane pair per (trajectory, axis) as the 8-lane shape (lane = trajectory * 8 + axis * 2 + side,
// axis 3 idle), and in step `step` every pair emits BOTH own segments 2 step and 2 step + 1 (sub = 0, 1) -- the segments the two lane pairs
// of the 16-lane shape emit in that step.  Staging: the eight trajectories are two HALVES of four, and a half is laid out exactly as the
// 16-lane tile of four trajectories is: one block of 16 rows per (half, axis), row `rest` of a block = twmap_rest<2>(trajectory of the
// half, sub, side).  Copy instruction `piece` (six per step) moves block `piece`: lane = rest * 4 + 16-byte column, so each of the six
// stores of a step writes what one store of the 16-lane kernel writes -- whole 128-byte lines for r = 4 and even M, each from eight
// adjacent lanes, 96-byte runs for r = 3, the two halves of the middle line in the last step where (M + 1) / 2 is odd.
#pragma once
#include "qp_twisted_map.h"

namespace uavqp {

static constexpr int TWMAP8_TILE = 8;      // trajectories of a wave
static constexpr int TWMAP8_PIECES = 6;    // copy instructions (16 bytes per lane each) of a step
static constexpr int TWMAP8_ROWS = 96;     // staging rows: 8 trajectories x 3 axes x 2 sides x 2 subs

// emission steps of a wave
UAVQP_MAP_HD constexpr int twmap8_steps(int M) { return twmap_steps<2>(M); }
// the producing lane of (trajectory of the tile, axis, side)
UAVQP_MAP_HD constexpr int twmap8_lane(int tl, int axis, int side) { return tl * 8 + axis * 2 + side; }
// block of 16 staging rows that (trajectory of the tile, axis) writes, and what copy instruction `piece` = block moves
UAVQP_MAP_HD constexpr int twmap8_block(int tl, int axis) { return (tl >> 2) * 3 + axis; }
UAVQP_MAP_HD constexpr int twmap8_block_half(int block) { return block / 3; }
UAVQP_MAP_HD constexpr int twmap8_block_axis(int block) { return block % 3; }
// row within the block
UAVQP_MAP_HD constexpr int twmap8_rest(int tl, int sub, int side) { return twmap_rest<2>(tl & 3, sub, side); }
// staging row 0 .. 95 of the chunk (trajectory of the tile, axis, side, sub)
UAVQP_MAP_HD constexpr int twmap8_row(int tl, int axis, int side, int sub) { return twmap8_block(tl, axis) * 16 + twmap8_rest(tl, sub, side); }

// Where the rows lie in LDS, in doubles from the start of the staging area.  A row holds up to 8 doubles at a stride of 10 (5 bank
// quads of 16 bytes), a block is 16 rows, linear in `rest` (the copy-out reads a block with one address per lane).  16 consecutive
// lanes are two trajectories of one half x three axes x two sides; their rows of one sub start 0 / 4 quads (trajectory) + 0 / 15 (sub 0)
// or 0 / 5 (sub 1) quads (side) apart, modulo the 16 quads of the 64 banks, so with the blocks of the three axes shifted by 0 / 2 / 8
// quads the twelve b128 writes start in twelve different bank quads.  The second half lies 10 quads further on; every block starts
// clear of the last row of the block in front, and the 16 rows behind the blocks take the writes of the idle lane pairs
// (a kernel whose idle pairs do not write allocates TWMAP8_IDLE_BASE doubles only: qp_twisted.h, TwistedCfg::IDLE_ROWS2).
static constexpr int TWMAP8_ROW_STRIDE = 10, TWMAP8_ROW_DOUBLES = 8;
UAVQP_MAP_HD constexpr int twmap8_block_base(int block) {
    return block * 16 * TWMAP8_ROW_STRIDE + twmap8_block_half(block) * 20 + (twmap8_block_axis(block) == 0 ? 0 : (twmap8_block_axis(block) == 1 ? 4 : 16));
}
UAVQP_MAP_HD constexpr int twmap8_row_addr(int block, int rest) { return twmap8_block_base(block) + rest * TWMAP8_ROW_STRIDE; }
static constexpr int TWMAP8_IDLE_BASE = TWMAP8_ROWS * TWMAP8_ROW_STRIDE + 40;
UAVQP_MAP_HD constexpr int twmap8_idle_addr(int idle_row) { return TWMAP8_IDLE_BASE + idle_row * TWMAP8_ROW_STRIDE; }   // idle_row 0 .. 15
static constexpr int TWMAP8_STAGE_DOUBLES = TWMAP8_IDLE_BASE + 16 * TWMAP8_ROW_STRIDE;

// The piece lane `lane` copies in step `step` with copy instruction `piece`.
struct TwistedPiece8 {
    int traj, axis, side, sub;   // producer: trajectory of the tile, axis, side, which of its two segments of the step
    int row;                     // staging row the piece is read from
    int segment;                 // global segment
    int col;                     // 16-byte column of the 2r-coefficient chunk
    bool keep;                   // false: the producer has no such segment, or the column is padding (r = 3) -- the store is dropped
    long long byte;              // offset in the tile's coefficients [traj][axis][segment][2r] of doubles; meaningful if keep
};
UAVQP_MAP_HD inline TwistedPiece8 twmap8_piece(int lane, int step, int piece, int M, int r) {
    const int rest = lane >> 2, nc = 2 * r;
    TwistedPiece8 p;
    p.col = lane & 3;
    p.traj = twmap8_block_half(piece) * 4 + twmap_rest_traj<2>(rest);
    p.axis = twmap8_block_axis(piece);
    p.side = twmap_rest_side<2>(rest);
    p.sub = twmap_rest_sub<2>(rest);
    p.row = piece * 16 + rest;
    const int jv = twmap_own_segment<2>(step, p.sub);
    p.segment = twmap_global_segment(M, p.side, jv);
    p.keep = p.col < nc / 2 && jv < twmap_side_segments(M, p.side);
    p.byte = ((((long long)p.traj * 3 + p.axis) * M + p.segment) * nc + 2 * p.col) * 8;
    return p;
}

}  // namespace uavqp
